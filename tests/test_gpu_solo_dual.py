"""GPU tests of the two-half form of the kinematic persistent kernel's evaluation (mpc_solo.hpp solo_halves, mpc_eval.hpp
kin_wide_rollout2): a trip that carries a speculative gradient serves the request on lanes 0 .. 31 and the speculative
gradient on lanes 32 .. 63 of the agent's wave.

Evaluation: "two points, one trip" (mpc_eval_cost_grad_wave2) against the same two points evaluated one at a time by
the 64-lane wave form (mpc_eval_cost_grad_wave) and by the round path's kernels (mpc_eval_cost_grad), bit for bit, at
horizons of one pass of 32 lanes, around a pass boundary, the benchmark's and the largest.  Every batch holds agents
whose stages are outside the fast range of the rollout in both halves, in one half alone (either one), and agents with a
non-finite control in one half alone.  Which half is outside is decided by the data: kin4_in_range bounds the heading
increment of a stage by h |v| |sin(beta) / lr|, which at v = 60 is beyond its limit for every steering angle but zero,
and zero for a steering angle of zero.

Solve: all in the persistent kernel, a switch to it in mid-solve and rounds only give the same controls and statistics;
the persistent kernel consumes speculative gradients, MPC_NO_SPEC switches them off without changing a bit, the
accounting identity of test_gpu_speculation.py holds, and a horizon beyond half a wave issues none."""
import numpy as np
import pytest
import torch

from conftest import straight_centerline, synthetic_states

pytestmark = pytest.mark.gpu

import model_predictive_control_amd as mp  # noqa: E402

SWITCHES = ("MPC_SPEC_POLICY", "MPC_SPEC_DEPTH", "MPC_CHAIN_MIN", "MPC_NO_CHAIN", "MPC_NO_SPEC", "MPC_SOLO_MAX", "MPC_SOLO_ALL",
            "MPC_LDS_PAIRS", "MPC_ALL_ROWS", "MPC_STEP_REGS")
B_EVAL = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)


def eval_problem(N):
    """x0 [64, 4] and two different control rows per agent, [64, 2 N] each; agent a is of class a % 8:
    0 both halves outside the fast range, 1 the second half alone, 2 the first half alone, 3 a NaN in the second row alone,
    4 a NaN in the first row alone, 5 .. 7 ordinary."""
    rng = np.random.default_rng(100 + N)
    x0 = synthetic_states(0, B_EVAL, seed=31)
    U1 = np.stack([rng.uniform(-1.0, 1.0, (B_EVAL, N)), rng.uniform(-0.3, 0.3, (B_EVAL, N))], 2)
    U2 = np.stack([rng.uniform(-1.0, 1.0, (B_EVAL, N)), rng.uniform(-0.3, 0.3, (B_EVAL, N))], 2)
    cls = np.arange(B_EVAL) % 8
    x0[cls <= 2, 3] = 60.0
    U1[cls == 1, :, 1] = 0.0
    U2[cls == 2, :, 1] = 0.0
    k = min(3, N - 1)
    U2[cls == 3, k, 1] = np.nan
    U1[cls == 4, 0, 0] = np.nan
    return x0, U1.reshape(B_EVAL, 2 * N), U2.reshape(B_EVAL, 2 * N), cls


@pytest.mark.parametrize("N", [1, 7, 8, 9, 20, 32])
def test_two_points_in_one_trip_are_the_two_evaluations(dev, N):
    x0, U1, U2, cls = eval_problem(N)
    eng = mp.BatchedMPC(mp.default_config(0, N), dev)
    X0, cl, U1t, U2t = T(x0, dev), T(straight_centerline(), dev), T(U1, dev), T(U2, dev)
    np_ = lambda t: t.cpu().numpy()
    ref = {}
    for wave in (True, False):
        p1, g1, _ = eng.eval_cost_grad(X0, cl, U1t, wave=wave)
        p2, g2, _ = eng.eval_cost_grad(X0, cl, U2t, wave=wave)
        pc, _, _ = eng.eval_cost_grad(X0, cl, U1t, want_grad=False, wave=wave)
        ref[wave] = (np_(p1), np_(g1), np_(g2), np_(pc))
    psi, grad, grad2, _ = eng.eval_cost_grad_pair(X0, cl, U1t, U2t)
    psic, none, grad2c, _ = eng.eval_cost_grad_pair(X0, cl, U1t, U2t, want_grad=False)
    assert none is None
    psi, grad, grad2, psic, grad2c = np_(psi), np_(grad), np_(grad2), np_(psic), np_(grad2c)
    eq = lambda a, b: np.array_equal(a, b, equal_nan=True)
    for wave in (True, False):
        p1, g1, g2, pc = ref[wave]
        assert eq(psi, p1) and eq(grad, g1), wave         # the request: cost and gradient at the first point
        assert eq(grad2, g2), wave                        # the speculative half: the gradient at the second point
        assert eq(psic, pc) and eq(grad2c, g2), wave      # a cost request beside the speculative gradient
    # the data is what the docstring says: a non-finite control spoils its own half and nothing else
    p1, g1, g2, _ = ref[True]
    clean = cls >= 5
    assert np.isfinite(p1[clean]).all() and np.isfinite(g1[clean]).all() and np.isfinite(g2[clean]).all()
    assert np.isfinite(g1[cls == 3]).all() and not np.isfinite(g2[cls == 3]).all()
    assert np.isfinite(g2[cls == 4]).all() and not np.isfinite(p1[cls == 4]).any()
    assert np.isfinite(g1[cls <= 2]).all() and np.isfinite(g2[cls <= 2]).all()
    assert not eq(g1, g2)


def solve(monkeypatch, dev, cfg, x0, N, solo_max=None, **env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    B = x0.shape[0]
    eng = mp.BatchedMPC(cfg, dev)
    if solo_max is not None:
        eng.set_solo_max(solo_max)
    U, _, st = eng.solve(T(x0, dev), T(straight_centerline(), dev), T(np.tile([1., 0.], (B, N)), dev))
    return U, st, eng.last_solve_info()


def identity_holds(st, info):
    return info["evals_grad"] + info["evals_cost"] == int(st[:, 7].sum()) + info["spec_issued"] - info["spec_used"]


@pytest.mark.parametrize("N,B", [(20, 64), (20, 700), (32, 100)])
def test_solve_is_bit_identical_on_every_path(dev, monkeypatch, N, B):
    x0 = synthetic_states(0, B, seed=17)
    x0[::23, 3] = 60.0                                    # outside the fast ranges of the wide rollout
    cfg = mp.default_config(0, N, max_total_inner=400, max_total_evals=3000)
    Ur, sr, ir = solve(monkeypatch, dev, cfg, x0, N, solo_max=0)                 # rounds only
    Ua, sa, ia = solve(monkeypatch, dev, cfg, x0, N, MPC_SOLO_ALL=4096)          # all in the persistent kernel
    Um, sm, im = solve(monkeypatch, dev, cfg, x0, N, solo_max=64)                # switch in mid-solve
    Un, sn, in_ = solve(monkeypatch, dev, cfg, x0, N, MPC_SOLO_ALL=4096, MPC_NO_SPEC=1)
    print({k: (ir[k], ia[k], im[k], in_[k]) for k in ("rounds", "solo_agents", "spec_issued", "spec_used", "evals_grad", "evals_cost")})
    assert ir["solo_agents"] == 0 and ir["rounds"] > 0
    assert ia["solo_agents"] == B and ia["rounds"] == 0
    assert in_["solo_agents"] == B and in_["rounds"] == 0
    assert im["solo_agents"] > 0
    if B > 64:
        assert im["solo_agents"] < B and im["rounds"] > 0
    for U, st in ((Ua, sa), (Um, sm), (Un, sn)):
        assert torch.equal(U, Ur) and torch.equal(st, sr)
    assert ia["spec_used"] > 0
    assert in_["spec_issued"] == 0 and in_["spec_used"] == 0
    for st, info in ((sr, ir), (sa, ia), (sm, im), (sn, in_)):
        assert identity_holds(st, info)
    assert (sr[:, 0] == 1).float().mean() >= 0.5 and torch.isfinite(Ur).all()


def test_horizon_beyond_half_a_wave_keeps_the_one_request_path(dev, monkeypatch):
    N, B = 40, 100
    x0 = synthetic_states(0, B, seed=17)
    x0[::23, 3] = 60.0
    cfg = mp.default_config(0, N, max_total_inner=400, max_total_evals=3000)
    Ur, sr, ir = solve(monkeypatch, dev, cfg, x0, N, solo_max=0)
    Ua, sa, ia = solve(monkeypatch, dev, cfg, x0, N, MPC_SOLO_ALL=4096)
    assert ir["solo_agents"] == 0 and ir["rounds"] > 0
    assert ia["solo_agents"] == B and ia["rounds"] == 0
    assert torch.equal(Ua, Ur) and torch.equal(sa, sr)
    assert ia["spec_issued"] == 0
    assert identity_holds(sa, ia) and identity_holds(sr, ir)
