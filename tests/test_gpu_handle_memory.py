"""GPU tests of the handle's memory at a second batch size (csrc/mpc_arena.hpp, the reserve_* calls of mpc_handle.hpp): an
engine whose arenas have grown -- or that holds more than a call needs -- returns the bits of a fresh engine, and the
nominal states of the event-triggered loop outlive a regrown staging arena.  Agents are independent and every run
repeats bit for bit (tests/test_gpu_parity.py), so every comparison is exact.  Kinematic model, N = 20, a short
iteration budget: equality of bits does not need converged agents."""
import numpy as np
import pytest
import torch

import discs_common as D
from agent_tables_common import T
from conftest import straight_centerline, synthetic_states

pytestmark = pytest.mark.gpu

import model_predictive_control_amd as mp  # noqa: E402

N = 20


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def same(a, b):
    """bit equality of two results: tuples of tensors (float64 by their bits) or None"""
    for u, v in zip(a, b):
        if u is None or v is None:
            assert u is None and v is None
        elif u.dtype == torch.float64:
            assert u.shape == v.shape and torch.equal(u.contiguous().view(torch.int64), v.contiguous().view(torch.int64))
        else:
            assert torch.equal(u, v)
    return True


@pytest.mark.parametrize("rounds", [False, True])
def test_solve_at_64_65_64_agents_is_a_fresh_engines(dev, rounds):
    """One engine solves 64, then 65, then 64 agents -- the workspace grows across the 64-agent padding and is then larger
    than the batch -- and every (U, lam, stats) is a fresh engine's on the same batch.  rounds: through the round path
    (lists, counters, K1 scratch) instead of the persistent kernel."""
    cfg = mp.default_config(mp.MODEL_KINEMATIC, N, max_total_inner=200, constr_mode=mp.CONSTR_STATE_SQ,
                            D_lb=[-np.inf] * 6, D_ub=[0.0] * 6, g_off=[20, 1, 1, 0.5, 1, 0.1], Sigma0=10.0)
    X0 = synthetic_states(0, 65, seed=5)
    X0[:, 0] *= 3.9 / 5.0
    X0[:, 3] = np.minimum(X0[:, 3], 0.65)
    cl = T(straight_centerline(), dev)

    def engine():
        e = mp.BatchedMPC(cfg, dev)
        if rounds:
            e.set_solo_max(0)
        return e

    def solve(e, B):
        return e.solve(T(X0[:B], dev), cl, T(np.tile([1., 0.], (B, N)), dev))

    fresh = {}
    for B in (64, 65):
        e = engine()
        fresh[B] = solve(e, B)
        assert (e.last_solve_info()["rounds"] > 0) == rounds
        e.close()
    eng = engine()
    for B in (64, 65, 64):
        assert same(solve(eng, B), fresh[B]), B
    eng.close()


def test_nominal_states_outlive_a_regrown_staging_arena(dev):
    """closed_loop_event at 66 agents (its staging arena holds 128), then a masked solve of no agent on a batch of 198 made
    of copies of the loop's x, U and lam -- it regrows the staging arena, runs no solve and writes nothing back -- then the
    loop again from the returned held: the second stretch is, bit for bit, that of an engine that skipped the middle call.
    (A masked solve of the loop's own 66 rows would fit the arena the loop has reserved: the copies are there to outgrow
    it.)  Between the stretches the trigger's decisions rest on the nominal states alone: lost, every agent would fire at
    once; kept, the agents fire as their hold limit comes."""
    B, T1, T2, thr, max_hold = 66, 3, 4, 0.05, 5
    cfg = mp.default_config(mp.MODEL_KINEMATIC, N, max_total_inner=60)
    x0, cl = T(synthetic_states(0, B, seed=9), dev), T(straight_centerline(), dev)
    U0 = T(np.tile([1., 0.], (B, N)), dev)
    w = np.ones(4)
    second = []
    for regrow in (False, True):
        eng = mp.BatchedMPC(cfg, dev)
        r1 = eng.closed_loop_event(x0, cl, U0, T1, w, thr, max_hold, shift=True)
        if regrow:
            x3, U3 = r1.x.repeat(3, 1), r1.U.repeat(3, 1)
            lam3 = None if r1.lam is None else r1.lam.repeat(3, 1)
            nobody = torch.zeros(3 * B, dtype=torch.int32, device=dev)
            U, lam, _, n = eng.solve_active(x3, cl, U3, nobody, lam=lam3)
            assert n == 0 and same((U, lam), (U3, lam3))
        r2 = eng.closed_loop_event(r1.x, cl, r1.U, T2, w, thr, max_hold, held=r1.held, lam=r1.lam, shift=True, stats=r1.stats)
        second.append(r2)
        eng.close()
    assert same(second[1], second[0])
    solved = second[0].solved
    assert not bool(solved[:, 0].any()) and bool(solved.any())      # nobody fires on entering the second stretch; the hold limit does


def test_traffic_loop_at_64_then_130_agents_is_a_fresh_engines(dev):
    """closed_loop_traffic in scenes of two at 64 and then at 130 agents on one engine (its plan and opponent buffers, the
    workspace and the handle's own tables all grow): the second result is a fresh engine's."""
    G, Tn, reach = 2, 3, 0.6
    cfg = mp.default_config(mp.MODEL_KINEMATIC, N, constr_mode=mp.CONSTR_DISCS, Sigma0=10.0, max_total_inner=300)
    rng = np.random.default_rng(4)

    def case(B):
        """pairs on the line centerline, the rear car 0.3 behind and faster: its plan runs into the front car's disc"""
        X0 = np.zeros((B, 4))
        X0[:, 0] = 1.2 + np.repeat(rng.uniform(0, 2.0, B // G), G) + np.tile([0.0, 0.3], B // G)
        X0[:, 1] = 0.5 + rng.uniform(-.04, .04, B)
        X0[:, 2] = rng.uniform(-.05, .05, B)
        X0[:, 3] = np.tile([1.0, 0.5], B // G)
        return T(X0, dev), torch.zeros(B, 2 * N, dtype=torch.float64, device=dev), T(rng.uniform(0.2, 0.24, B), dev)

    cl = T(D.line_centerline(), dev)
    small, large = case(64), case(130)
    eng, fresh = mp.BatchedMPC(cfg, dev), mp.BatchedMPC(cfg, dev)
    x, U, r = small
    eng.closed_loop_traffic(x, cl, U, Tn, G, r, reach, shift=True)
    x, U, r = large
    got = eng.closed_loop_traffic(x, cl, U, Tn, G, r, reach, shift=True)
    want = fresh.closed_loop_traffic(x, cl, U, Tn, G, r, reach, shift=True)
    assert same(tuple(got), tuple(want))
    assert bool((got.traj_opp >= 0).any())                                    # opponents were chosen: the loop's buffers were in use
    eng.close(); fresh.close()
