"""GPU tests of lap driving (mpc_track_windows, mpc_track_locate, mpc_track_select, mpc_closed_loop_track): the windows
and the two placements against their numpy restatement over the oracle's nearest point (tests/track_loop_common.py),
the loop EXACTLY against existing entry points -- mpc_closed_loop_event on a one-window track, a host loop built from
track_select, trigger_eval, solve_active and rollout in general -- and against the CPU oracle's mirror loop on a case that
crosses the seam of a closed track."""
import ctypes as C

import numpy as np
import pytest
import torch

import event_loop_common as E
import track_loop_common as K
from conftest import straight_centerline, synthetic_states

pytestmark = pytest.mark.gpu

import model_predictive_control_amd as mp  # noqa: E402
from model_predictive_control_amd import _lib  # noqa: E402
from model_predictive_control_amd.tracks import stadium_track, circle_track  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def T(a, dev, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def track_poses(track, B, seed, model, lateral=0.3):
    """B states beside random points of a track: up to `lateral` to either side, heading within 0.3 rad of the
    tangent, the speeds of conftest.synthetic_states"""
    rng = np.random.default_rng(seed)
    L = track.size // 2
    x, y = track[:L], track[L:]
    i = rng.integers(0, L, B)
    tx, ty = x[(i + 1) % L] - x[i], y[(i + 1) % L] - y[i]
    nrm = np.hypot(tx, ty)
    tx, ty = tx / nrm, ty / nrm
    d = rng.uniform(-lateral, lateral, B)
    cols = [x[i] - d * ty, y[i] + d * tx, np.arctan2(ty, tx) + rng.uniform(-.3, .3, B), rng.uniform(.3, 1.5, B)]
    if model == 1:
        cols += [rng.uniform(-.05, .05, B), rng.uniform(-.5, .5, B)]
    return np.stack(cols, 1)


# ----------------------------------------------------------------------------- 1. windows
@pytest.mark.parametrize("closed,S,L,stride,Kt", [
    (True, 100, 388, 4, 3), (False, 100, 388, 4, 3),      # the seam case's geometry, three tracks
    (True, 100, 389, 7, 1), (False, 100, 389, 7, 2),      # L no multiple of the stride
    (True, 37, 101, 5, 3), (False, 37, 101, 5, 3),        # S = 37
    (True, 100, 100, 3, 1), (False, 100, 100, 3, 2),      # L = S: the open track has one window
    (True, 37, 37, 40, 2), (False, 37, 2000, 1, 1),       # a stride beyond the track; stride 1 (1 964 windows)
])
def test_windows_are_the_numpy_gather(dev, closed, S, L, stride, Kt):
    eng = mp.BatchedMPC(mp.default_config(0, 20, S=S), dev)
    track = np.random.default_rng(L + stride).normal(0, 3, (Kt, 2 * L))
    g = K.geom(Kt, L, S, stride, 1, closed)
    trk = eng.track_windows(T(track, dev), stride, 1, closed)
    assert (trk.K, trk.L, trk.S, trk.stride, trk.lead, trk.closed, trk.R) == (Kt, L, S, stride, 1, closed, g.R)
    assert not closed or L != S or g.R == -(-L // stride)
    if not closed and L == S:
        assert trk.R == 1
    assert same_bits(trk.win, T(K.windows(track, g), dev))
    eng.close()


# ----------------------------------------------------------------------------- 2. select, 3. locate
def select_case(closed, model=0, S=100):
    """two tracks (a stadium and a circle of as many points), 4 096 agents: three quarters beside a candidate point of
    their row, one quarter anywhere within 12 m of the origin (well off the track, partly outside a row's grid); rows
    anywhere, the last row of each track and -- closed -- the rows whose window spans the seam included"""
    B = 4096
    st = stadium_track(10, 3, 0.1)
    L = st.size // 2
    track = np.stack([st, circle_track(L, 5.0) + np.r_[np.full(L, 20.0), np.zeros(L)]])
    g = K.geom(2, L, S, 4, 10, closed)
    win = K.windows(track, g)
    rng = np.random.default_rng(7 + closed)
    rows = rng.integers(0, g.K * g.R, B)
    rows[:64] = g.R - 1                                           # the last row of track 0
    rows[64:128] = 2 * g.R - 1                                    # ... and of track 1
    if closed:
        seam = np.flatnonzero((np.arange(g.R) * g.stride + S - 1) >= L)
        assert seam.size > 10
        rows[128:512] = rng.choice(seam, 384) + g.R * rng.integers(0, 2, 384)
    i = rng.integers(0, S - 1, B)
    x = synthetic_states(model, B, seed=3)
    x[:, 0] = win[rows, i] + rng.uniform(-.3, .3, B)
    x[:, 1] = win[rows, S + i] + rng.uniform(-.3, .3, B)
    far = rng.random(B) < 0.25
    far[:128] = False
    x[far, 0] = rng.uniform(-12, 32, far.sum())
    x[far, 1] = rng.uniform(-12, 12, far.sum())
    return track, g, win, rows, x


@pytest.mark.parametrize("grid", [True, False])
@pytest.mark.parametrize("closed", [True, False])
def test_select_equals_the_rule_over_the_oracle_nearest(dev, O, closed, grid):
    track, g, win, rows, x = select_case(closed)
    B = len(rows)
    eng = mp.BatchedMPC(mp.default_config(0, 20), dev)
    eng.set_nearest_blocks(grid)
    trk = eng.track_windows(T(track, dev), g.stride, g.lead, closed)
    assert same_bits(trk.win, T(win, dev))
    ocfg = O.default_config(0, 20)
    want_rows, want_pos = K.select(O, ocfg, x, win, rows, g)
    assert (want_rows != rows).mean() > 0.5 and (want_pos >= 0).all()
    if closed:
        assert (want_rows % g.R < rows % g.R - g.R // 2).any()       # some agents move across the seam
    else:
        assert (want_rows % g.R == g.R - 1).any() and (want_rows % g.R == 0).any()    # both clamps
    ci, pos = eng.track_select(T(x, dev), trk, T(rows, dev, torch.int32))
    assert np.array_equal(ci.cpu().numpy(), want_rows) and np.array_equal(pos.cpu().numpy(), want_pos)
    # masked agents and non-finite poses are untouched (pos keeps the -1 the front end fills in)
    rng = np.random.default_rng(11)
    act = rng.random(B) < 0.6
    xb = x.copy()
    xb[5::17, 0] = np.nan
    xb[6::17, 1] = np.inf
    xb[7::17, 1] = -np.inf
    with np.errstate(invalid="ignore"):
        want_rows, want_pos = K.select(O, ocfg, xb, win, rows, g, active=act)
    skipped = ~act | ~np.isfinite(xb[:, :2]).all(1)
    assert np.array_equal(want_rows[skipped], rows[skipped]) and (want_pos[skipped] == -1).all() and skipped.sum() > 1000
    for mask in (T(act, dev, torch.bool), T(act.astype(np.int32) * 5, dev, torch.int32)):
        ci, pos = eng.track_select(T(xb, dev), trk, T(rows, dev, torch.int32), active=mask)
        assert np.array_equal(ci.cpu().numpy(), want_rows) and np.array_equal(pos.cpu().numpy(), want_pos)
    # the raw call: pos may be NULL, a row that is not a row of the table is not written
    p = lambda t: C.c_void_p(t.data_ptr())
    xd, cd = T(x, dev), T(rows, dev, torch.int32)
    cd[:3] = torch.tensor([-1, g.K * g.R, 2 ** 30], dtype=torch.int32, device=dev)
    assert eng.lib.mpc_track_select(eng._h, C.byref(trk._c), B, p(xd), p(trk.win), None, p(cd), None, None) == 0
    got = cd.cpu().numpy()
    assert list(got[:3]) == [-1, g.K * g.R, 2 ** 30] and np.array_equal(got[3:], K.select(O, ocfg, x, win, rows, g)[0][3:])
    with pytest.raises(ValueError):
        eng.track_select(xd, trk, cd)                                  # the front end checks the range
    eng.close()


@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("model", [0, 1])
def test_locate_equals_the_oracle_whole_track_nearest(dev, O, closed, model):
    track, g, win, _, x = select_case(closed, model)
    B = len(x)
    eng = mp.BatchedMPC(mp.default_config(model, 12), dev)
    trk = eng.track_windows(T(track, dev), g.stride, g.lead, closed)
    ti = np.random.default_rng(2).integers(0, 2, B)
    ocfgL = O.default_config(model, 12, S=g.L)
    want = K.locate(O, ocfgL, x, track, g, ti)
    got = eng.track_locate(T(x, dev), trk, T(ti, dev, torch.int32)).cpu().numpy()
    assert np.array_equal(got, want) and len(np.unique(want)) > g.R
    got0 = eng.track_locate(T(x, dev), trk).cpu().numpy()               # None: track 0
    assert np.array_equal(got0, K.locate(O, ocfgL, x, track, g)) and got0.max() < g.R
    # an agent ON a track point is placed with that point at index `lead` .. lead + w - 1 of its row (where not clamped)
    # (point L-1 is no candidate and, on a closed track, as far from L-2 as from 0: left out)
    a = np.arange(g.L - 1)
    xs = np.zeros((g.L - 1, eng.nx))
    xs[:, 0], xs[:, 1] = track[0, a], track[0, g.L + a]
    rows = eng.track_locate(T(xs, dev), trk).cpu().numpy()
    idx = (a - rows * g.stride) % g.L if closed else a - rows * g.stride
    inside = np.ones(g.L - 1, bool) if closed else ((a - g.lead) // g.stride >= 0) & ((a - g.lead) // g.stride <= g.R - 1)
    assert ((idx[inside] >= g.lead) & (idx[inside] < g.lead + g.stride)).all() and inside.sum() > 200
    with pytest.raises(ValueError):
        eng.track_locate(T(x, dev), trk, T(ti + 1, dev, torch.int32))
    eng.close()


# ----------------------------------------------------------------------------- 4. one window
@pytest.mark.parametrize("model,N", [(0, 20), (1, 12)])
def test_one_window_track_is_the_event_loop(dev, model, N):
    """An open track with L = S has one window, the centerline itself: closed_loop_track is closed_loop_event on that row,
    bit for bit (controls, trajectories, stats, held), whether the event loop is given the row index or none"""
    B, Tn, thr, max_hold = 192, 12, 0.02, 5
    eng = mp.BatchedMPC(mp.default_config(model, N, max_total_inner=1500), dev)
    cl = T(straight_centerline(), dev)
    trk = eng.track_windows(cl, 4, 10, False)
    assert trk.R == 1 and same_bits(trk.win, cl[None, :])
    x0, U0 = T(synthetic_states(model, B, seed=8), dev), T(np.tile([1., 0.], (B, N)), dev)
    dist = T(np.random.default_rng(5).normal(0, 4e-3, (B, Tn, eng.nx)), dev)
    w = np.ones(eng.nx)
    zero = torch.zeros(B, dtype=torch.int32, device=dev)
    assert torch.equal(eng.track_locate(x0, trk), zero)
    r = eng.closed_loop_track(x0, trk, U0, Tn, w, thr, max_hold, zero, shift=True, disturbance=dist)
    assert bool((r.cl_index == 0).all()) and bool((r.traj_row == 0).all())
    assert 0.05 < float(r.solved.float().mean()) < 0.9
    for ci in (zero, None):
        e = eng.closed_loop_event(x0, trk.win, U0, Tn, w, thr, max_hold, shift=True, disturbance=dist, cl_index=ci)
        assert same_bits(r.traj_u, e.traj_u) and same_bits(r.traj_x, e.traj_x) and same_bits(r.x, e.x)
        assert same_bits(r.U, e.U) and same_bits(r.stats, e.stats)
        assert torch.equal(r.held, e.held) and torch.equal(r.solved, e.solved)
        assert torch.equal(r.solve_count, e.solve_count) and torch.equal(r.failures, e.failures)
    eng.close()


# ----------------------------------------------------------------------------- 5. the host loop
def host_track_loop(eng, trk, x, ci, U, Tn, w, thr, max_hold, shift, plant=None, dist=None):
    """mpc_closed_loop_track from the host: trigger_eval, track_select of the firing agents, the shift in torch,
    solve_active, rollout(Nsim = 1).  plant = (table, index, plant_index) when a table is bound."""
    B, N, nx, dev = x.shape[0], eng.N, eng.nx, x.device
    x, U, ci = x.clone(), U.clone(), ci.clone()
    held = torch.full((B,), -1, dtype=torch.int32, device=dev)
    xhat = torch.zeros_like(x)
    stats = torch.zeros(B, 8, dtype=torch.float64, device=dev)
    solved = torch.zeros(B, Tn, dtype=torch.uint8, device=dev)
    tx, tu = torch.zeros(B, Tn, nx, dtype=torch.float64, device=dev), torch.zeros(B, Tn, 2, dtype=torch.float64, device=dev)
    trow = torch.zeros(B, Tn, dtype=torch.int32, device=dev)
    ar, stage = torch.arange(B, device=dev), torch.arange(N, device=dev)
    for t in range(Tn):
        _, fire = eng.trigger_eval(x, xhat, held, w, thr, max_hold)
        fb = fire != 0
        ci, _ = eng.track_select(x, trk, ci, active=fire)
        if shift:
            src = torch.clamp(stage[None, :] + torch.clamp(held, min=0)[:, None].long(), max=N - 1)
            Us = torch.gather(U.view(B, N, 2), 1, src[:, :, None].expand(B, N, 2)).reshape(B, 2 * N)
            U = torch.where(fb[:, None], Us, U)
        U, _, stats, n = eng.solve_active(x, trk.win, U, fire, stats=stats, cl_index=ci)
        assert n == int(fb.sum())
        held = torch.where(fb, torch.zeros_like(held), held)
        xhat = torch.where(fb[:, None], x, xhat)
        u = U.view(B, N, 2)[ar, held.long()].contiguous()
        if plant is not None:
            eng.set_agent_params(plant[0], plant[2])
        xn = eng.rollout(x, u)[:, 0]
        if plant is not None:
            eng.set_agent_params(*plant)
        x = ((xn + dist[:, t]) if dist is not None else xn).contiguous()
        xhat = eng.rollout(xhat, u)[:, 0].contiguous()
        held = held + 1
        solved[:, t], tx[:, t], tu[:, t], trow[:, t] = fb.to(torch.uint8), x, u, ci
    return dict(x=x, U=U, held=held, solved=solved, traj_x=tx, traj_u=tu, stats=stats, cl_index=ci, traj_row=trow)


def host_loop_case(dev, B, Tn, table, split=None):
    """(The iteration budget is short: equality of bits does not need converged agents, and on the curves of the stadium
    the slowest agent of a solve, not the batch, sets the time of a step.)"""
    N, model, thr, max_hold = 20, 0, 0.02, 10
    cfg = mp.default_config(model, N, max_total_inner=150)
    eng = mp.BatchedMPC(cfg, dev)
    track = stadium_track(10, 3, 0.1)
    trk = eng.track_windows(T(track, dev), 4, 10, True)
    assert trk.R == 97
    x0 = T(track_poses(track, B, 13, model), dev)
    U0, w = T(np.tile([1., 0.], (B, N)), dev), np.array([1.0, 1.0, 0.5, 0.25])
    dist = T(np.random.default_rng(17).normal(0, 4e-3, (B, Tn, 4)) * [1, 1, 0.5, 2], dev)
    plant = None
    if table:
        tab = T(_lib.param_rows(cfg, 3, accel=[2.0, 2.0 * 0.97, 2.0 * 1.02], friction=[1.0, 1.1, 0.93]), dev)
        plant = (tab, torch.zeros(B, dtype=torch.int32, device=dev), T(1 + np.arange(B) % 2, dev, torch.int32))
        eng.set_agent_params(*plant)
    ci0 = eng.track_locate(x0, trk)
    assert len(torch.unique(ci0)) > 90                            # the agents are spread over the whole track
    r = eng.closed_loop_track(x0, trk, U0, Tn, w, thr, max_hold, ci0, shift=True, disturbance=dist)
    frac = float(r.solved.float().mean())
    moved = float((r.cl_index != ci0).float().mean())
    print(f"B {B} table {table}: solve fraction {frac:.3f}, agents on another row at the end {moved:.3f}")
    assert 0.05 < frac < 0.9 and (moved > 0.5 or Tn < 20)
    assert torch.equal(r.traj_row[:, -1], r.cl_index) and torch.equal(r.solve_count, r.solved.sum(1).to(torch.int32))
    # an agent's row changes only at a step at which it is solved
    changed = r.traj_row[:, 1:] != r.traj_row[:, :-1]
    assert not bool((changed & (r.solved[:, 1:] == 0)).any())
    hl = host_track_loop(eng, trk, x0, ci0, U0, Tn, w, thr, max_hold, True, plant=plant, dist=dist)
    assert torch.equal(r.solved, hl["solved"]) and torch.equal(r.held, hl["held"])
    assert torch.equal(r.traj_row, hl["traj_row"]) and torch.equal(r.cl_index, hl["cl_index"])
    assert same_bits(r.traj_x, hl["traj_x"]) and same_bits(r.traj_u, hl["traj_u"]) and same_bits(r.x, hl["x"])
    assert same_bits(r.U, hl["U"]) and same_bits(r.stats, hl["stats"])
    if split:
        a = eng.closed_loop_track(x0, trk, U0, split, w, thr, max_hold, ci0, shift=True, disturbance=dist[:, :split].contiguous())
        b = eng.closed_loop_track(a.x, trk, a.U, Tn - split, w, thr, max_hold, a.cl_index, held=a.held, shift=True,
                                  stats=a.stats, disturbance=dist[:, split:].contiguous())
        assert same_bits(torch.cat([a.traj_x, b.traj_x], 1), r.traj_x) and same_bits(torch.cat([a.traj_u, b.traj_u], 1), r.traj_u)
        assert torch.equal(torch.cat([a.solved, b.solved], 1), r.solved) and torch.equal(torch.cat([a.traj_row, b.traj_row], 1), r.traj_row)
        assert torch.equal(a.solve_count + b.solve_count, r.solve_count) and torch.equal(a.failures + b.failures, r.failures)
        assert torch.equal(b.held, r.held) and torch.equal(b.cl_index, r.cl_index)
        assert same_bits(b.x, r.x) and same_bits(b.U, r.U) and same_bits(b.stats, r.stats)
    eng.close()


@pytest.mark.parametrize("table", [False, True])
def test_track_loop_equals_host_loop_4096_agents(dev, table):
    """... and a call with T = 25 followed by one with T = 15 equals one call with T = 40"""
    host_loop_case(dev, 4096, 40, table, split=25)


def test_track_loop_equals_host_loop_65536_agents(dev):
    host_loop_case(dev, 65536, 8, False)


# ----------------------------------------------------------------------------- 6. the oracle, across the seam
# The bound on |traj_x(HIP) - traj_x(oracle)| of the seam case: 100 times the larger of (a) that difference as measured
# on the MI355X (profiles/r12_track_loop.txt) and (b) the difference of two oracle runs whose evaluations differ by two
# ulps (eval_jitter(2, 5), printed by tests/test_track_loop_cpu.py) -- the recipe of TRAJ_X_BOUND in
# tests/test_gpu_event_loop.py.  Per model {0: kinematic N = 20, 1: Pacejka N = 12}, each the larger of thr = 0 and 0.02;
# measured (a): 9.2e-11 / 3.0e-10 kinematic, 5.9e-9 / 4.3e-9 Pacejka.  The bounds: 3.0e-8 and 6.1e-7.
HIP_VS_ORACLE_TRAJ_X = {0: 2.98e-10, 1: 5.86e-9}
JITTERED_ORACLE_TRAJ_X = {0: 1.92e-10, 1: 6.07e-9}      # the larger of thr = 0 and thr = 0.02
SEAM_TRAJ_X_BOUND = {m: 100.0 * max(HIP_VS_ORACLE_TRAJ_X[m], JITTERED_ORACLE_TRAJ_X[m]) for m in (0, 1)}
DU_METRIC = 1e-5      # bench.DU_METRIC: the project's bound on controls against the oracle


@pytest.mark.parametrize("thr", K.SEAM_THRESHOLDS)
@pytest.mark.parametrize("model,N", K.SEAM_MODELS)
def test_track_loop_matches_oracle_mirror_across_the_seam(dev, O, model, N, thr):
    ref = K.seam_mirror(O, model, N, thr)
    # the conditions, on the oracle alone (tests/test_track_loop_cpu.py checks them without a GPU)
    assert ref["fails"].sum() == 0 and ref["seam_crossings"] >= 1 and ref["gap"] > 1e-4
    assert thr == 0 or ref["margin"] > 1e-3
    X0, track, U0, w, g = K.seam_case(model, N)
    eng = mp.BatchedMPC(mp.default_config(model, N, **E.SOLVER), dev)
    trk = eng.track_windows(T(track, dev), g.stride, g.lead, True)
    ci0 = eng.track_locate(T(X0, dev), trk)
    assert np.array_equal(ci0.cpu().numpy(), K.locate(O, O.default_config(model, N, S=g.L), X0, track, g))
    r = eng.closed_loop_track(T(X0, dev), trk, T(U0, dev), K.SEAM["T"], w, thr, K.SEAM["max_hold"], ci0,
                              shift=bool(K.SEAM["shift"]))
    tx, tu = r.traj_x.cpu().numpy(), r.traj_u.cpu().numpy()
    du = np.abs(tu - ref["traj_u"]).max((1, 2)) / np.maximum(1.0, np.abs(ref["traj_u"]).max((1, 2)))
    dx = np.abs(tx - ref["traj_x"]).max()
    print(f"model {model} thr {thr}: solves {int(ref['solved'].sum())}, row changes {ref['row_changes']}, seam crossings "
          f"{ref['seam_crossings']}, gap {ref['gap']:.2e}; max rel |traj_u - oracle| = {du.max():.3e}, "
          f"max |traj_x - oracle| = {dx:.3e} (bound {SEAM_TRAJ_X_BOUND[model]:.1e})")
    assert np.array_equal(r.traj_row.cpu().numpy(), ref["traj_row"])          # decision for decision
    assert np.array_equal(r.cl_index.cpu().numpy(), ref["rows"])
    assert np.array_equal(r.solved.cpu().numpy() != 0, ref["solved"])
    assert np.array_equal(r.held.cpu().numpy(), ref["held"]) and int(r.failures.sum()) == 0
    assert du.max() <= DU_METRIC
    assert dx <= SEAM_TRAJ_X_BOUND[model]
    eng.close()


# ----------------------------------------------------------------------------- 7. more than a window
def test_agents_drive_past_the_end_of_their_first_window(dev):
    """An open straight track of 400 points (four centerlines long), 16 agents, 150 steps: every solve converges, every
    agent ends beyond point S of the track -- where a fixed row would have held it at S - 2 -- and its cross-track error
    on its final row is within what the same agents show at t = 20."""
    N, B, Tn, L = 20, 16, 150, 400
    eng = mp.BatchedMPC(mp.default_config(0, N, **E.SOLVER), dev)
    trk = eng.track_windows(T(straight_centerline(L), dev), 4, 10, False)
    X0 = synthetic_states(0, B, seed=1)
    X0[:, 0] += 4.0                                       # x in [4, 9] m: 7.5 m at v_ref end between 11.5 and 16.5 m
    x0, U0 = T(X0, dev), T(np.tile([1., 0.], (B, N)), dev)
    ci0 = eng.track_locate(x0, trk)
    r = eng.closed_loop_track(x0, trk, U0, Tn, np.ones(4), 0.0, 10, ci0, shift=True)
    assert int(r.failures.sum()) == 0 and bool((r.solve_count == Tn).all())
    _, pos = eng.track_select(r.x, trk, r.cl_index)
    pos = pos.cpu().numpy()
    print("final pos", pos, "rows", r.cl_index.cpu().numpy())
    assert (pos > eng.S).all() and (pos < L - 2).all()
    assert bool((r.cl_index > ci0).all())
    rows = r.traj_row.cpu().numpy()
    assert (np.diff(rows, axis=1) >= 0).all()             # nobody moves backwards on a straight
    err_end, _ = eng.stage_errors(r.x[:, :3].contiguous(), trk.win, r.cl_index)
    err_20, _ = eng.stage_errors(r.traj_x[:, 20, :3].contiguous(), trk.win, r.traj_row[:, 20].contiguous())
    cte_end, cte_20 = float(err_end[:, 0].abs().max()), float(err_20[:, 0].abs().max())
    print(f"max |cte| at t = 20: {cte_20:.3e}, at the end: {cte_end:.3e}")
    assert cte_end <= cte_20
    eng.close()


# ----------------------------------------------------------------------------- 8. refusals
def test_refusals(dev):
    N, B = 20, 64
    cfg = mp.default_config(0, N, max_total_inner=300)
    eng = mp.BatchedMPC(cfg, dev)
    track = T(stadium_track(10, 3, 0.1), dev)
    trk = eng.track_windows(track, 4, 10, True)
    x, U = T(track_poses(stadium_track(10, 3, 0.1), B, 1, 0), dev), T(np.tile([1., 0.], (B, N)), dev)
    ci = eng.track_locate(x, trk)
    p = lambda t: C.c_void_p(t.data_ptr())
    L_, h = eng.lib, eng._h
    w4 = (C.c_double * 4)(1, 1, 1, 1)
    held = torch.full((B,), -1, dtype=torch.int32, device=dev)

    def loop(t, b=B, cidx=ci):
        tp = None if t is None else C.byref(t)
        return L_.mpc_closed_loop_track(h, b, 2, 0, w4, 0.0, 1, p(x), p(trk.win), None if cidx is None else p(cidx), p(U), None,
                                        p(held), None, None, None, None, None, None, None, None, tp, None)
    # bad geometry: a track that is not what mpc_track_init gives for this handle
    for field, val in (("R", trk.R + 1), ("R", 0), ("stride", 5), ("L", 99), ("lead", 99), ("lead", -1), ("K", 0), ("closed", 2)):
        bad = _lib.MpcTrack(trk.K, trk.L, trk.stride, trk.lead, int(trk.closed), trk.R)
        setattr(bad, field, val)
        win = torch.zeros_like(trk.win)
        assert L_.mpc_track_windows(h, C.byref(bad), p(track), p(win), None) == -1, field
        assert L_.mpc_track_select(h, C.byref(bad), B, p(x), p(trk.win), None, p(ci.clone()), None, None) == -1, field
        assert L_.mpc_track_locate(h, C.byref(bad), B, p(x), p(track), None, p(ci.clone()), None) == -1, field
        assert loop(bad) == -1 and "geometry" in L_.mpc_last_error().decode(), field
    # a null track, null buffers
    assert L_.mpc_track_windows(h, None, p(track), p(trk.win), None) == -1
    assert L_.mpc_track_select(h, None, B, p(x), p(trk.win), None, p(ci.clone()), None, None) == -1
    assert L_.mpc_track_locate(h, None, B, p(x), p(track), None, p(ci.clone()), None) == -1
    assert loop(None) == -1 and "null track" in L_.mpc_last_error().decode()
    assert loop(trk._c, cidx=None) == -1                                       # cl_index is required
    assert L_.mpc_track_select(h, C.byref(trk._c), B, None, p(trk.win), None, p(ci.clone()), None, None) == -1
    assert L_.mpc_track_windows(h, C.byref(trk._c), None, p(trk.win), None) == -1
    # the front end: geometry, ranges, shapes
    for bad in (dict(stride=0), dict(lead=99), dict(lead=-1)):
        with pytest.raises(ValueError):
            eng.track_windows(track, **dict(dict(stride=4, lead=10, closed=True), **bad))
    with pytest.raises(ValueError):
        eng.track_windows(track[:150].contiguous(), 4, 10, True)              # L = 75 < S
    with pytest.raises(ValueError):
        eng.closed_loop_track(x, trk, U, 2, np.ones(4), 0.0, 1, ci + trk.R)    # rows out of range
    with pytest.raises(ValueError):
        eng.closed_loop_track(x, trk, U, 2, np.ones(4), 0.0, 1, None)
    with pytest.raises(TypeError):
        eng.closed_loop_track(x, trk.win, U, 2, np.ones(4), 0.0, 1, ci)
    # a batch size other than a bound table's
    tab = T(_lib.param_rows(cfg, 2), dev)
    idx = torch.zeros(B, dtype=torch.int32, device=dev)
    eng.set_agent_params(tab, idx)
    assert loop(trk._c) == 0
    assert loop(trk._c, b=B - 1) == -1 and "parameter table" in L_.mpc_last_error().decode()
    assert L_.mpc_track_select(h, C.byref(trk._c), B - 1, p(x), p(trk.win), None, p(ci.clone()), None, None) == -1
    assert L_.mpc_track_locate(h, C.byref(trk._c), B - 1, p(x), p(track), None, p(ci.clone()), None) == -1
    eng.clear_agent_params()
    btab = T(_lib.bound_rows(cfg, 1), dev)
    eng.set_agent_bounds(btab, idx)
    assert loop(trk._c, b=B - 1) == -1 and "bounds table" in L_.mpc_last_error().decode()
    eng.clear_agent_bounds()
    assert loop(trk._c, b=B - 1) == 0
    # refused while an asynchronous solve is in flight
    wait = eng.solve_async(x, trk.win, U, cl_index=ci)
    assert L_.mpc_track_select(h, C.byref(trk._c), B, p(x), p(trk.win), None, p(ci.clone()), None, None) == -1
    assert "in flight" in L_.mpc_last_error().decode()
    assert L_.mpc_track_windows(h, C.byref(trk._c), p(track), p(torch.zeros_like(trk.win)), None) == -1
    assert L_.mpc_track_locate(h, C.byref(trk._c), B, p(x), p(track), None, p(ci.clone()), None) == -1
    assert loop(trk._c) == -1 and "in flight" in L_.mpc_last_error().decode()
    with pytest.raises(_lib.MpcError):
        eng.track_select(x, trk, ci)
    wait()
    assert loop(trk._c) == 0
    eng.close()
