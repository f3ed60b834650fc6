"""GPU tests of MPC_SPEC_POLICY: which speculative Hessian-vector gradients the state machine does not issue.

Policy 0 issues one whenever its point exists.  Policy 1 leaves out those that the line-search condition or the stop
test -- both decided by numbers the agent holds before it would issue the gradient -- throw away: exact predictions, so
controls, statistics, rounds and the number of CONSUMED speculative gradients are those of policy 0 and only the number
issued falls.  Policy 2 also leaves out those of descent-lemma retries in launches that carry chain blocks (a policy, not a
prediction: same controls and statistics, fewer wasted gradients, possibly more rounds).  Everything is compared bit for
bit; the accounting identity of the round path, evals_grad + evals_cost == sum(stats[:, 7]) + spec_issued - spec_used,
holds under every policy.  The wave-per-agent form of PH_W_LS_G and the thread-per-agent one (chain blocks,
MPC_CHAIN_MIN=1) are both exercised."""
import numpy as np
import pytest
import torch

from conftest import straight_centerline, synthetic_states

pytestmark = pytest.mark.gpu

import model_predictive_control_amd as mp  # noqa: E402

SWITCHES = ("MPC_SPEC_POLICY", "MPC_SPEC_DEPTH", "MPC_CHAIN_MIN", "MPC_NO_CHAIN", "MPC_NO_SPEC", "MPC_SOLO_MAX", "MPC_SOLO_ALL",
            "MPC_LDS_PAIRS", "MPC_ALL_ROWS", "MPC_STEP_REGS")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)


def solve(monkeypatch, dev, cfg, x0, N, **env):
    """One solve on a fresh handle (the switches are read when it is created) with exactly the switches of `env` set."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    B = x0.shape[0]
    eng = mp.BatchedMPC(cfg, dev)
    U, lam, st = eng.solve(T(x0, dev), T(straight_centerline(), dev), T(np.tile([1., 0.], (B, N)), dev))
    return U, lam, st, eng.last_solve_info()


def identity_holds(st, info):
    return info["evals_grad"] + info["evals_cost"] == int(st[:, 7].sum()) + info["spec_issued"] - info["spec_used"]


def same(a, b):
    return (a is None and b is None) or torch.equal(a, b)


@pytest.fixture(scope="module")
def kin_round_runs(dev):
    """(a), (b): the kinematic round path, 300 agents, without and with chain blocks, policies 0, 1 and 2 (the default retry
    depth; key (True, 22): depth 2) -- solved once."""
    mpatch = pytest.MonkeyPatch()
    N, x0 = 20, synthetic_states(0, 300, seed=5)
    cfg = mp.default_config(0, N, max_total_inner=600)
    runs = {}
    try:
        for chain in (False, True):
            for policy in (0, 1) + ((2,) if chain else ()):
                env = dict(MPC_SOLO_MAX=0, MPC_SPEC_POLICY=policy)
                if chain:
                    env["MPC_CHAIN_MIN"] = 1
                runs[chain, policy] = solve(mpatch, dev, cfg, x0, N, **env)
        runs[True, 22] = solve(mpatch, dev, cfg, x0, N, MPC_SOLO_MAX=0, MPC_SPEC_POLICY=2, MPC_SPEC_DEPTH=2, MPC_CHAIN_MIN=1)
    finally:
        mpatch.undo()
    return runs


@pytest.mark.parametrize("chain", [False, True])
def test_exact_predictors_drop_only_unused_speculation(kin_round_runs, chain):
    U0, _, st0, i0 = kin_round_runs[chain, 0]
    U1, _, st1, i1 = kin_round_runs[chain, 1]
    print(chain, {k: (i0[k], i1[k]) for k in ("rounds", "spec_issued", "spec_used", "evals_grad", "evals_cost")})
    assert i0["rounds"] > 0 and i0["solo_agents"] == 0 and (st0[:, 0] == 1).all()
    assert torch.equal(U0, U1) and torch.equal(st0, st1)
    assert i1["rounds"] == i0["rounds"] and i1["spec_used"] == i0["spec_used"] > 0
    assert i1["spec_issued"] < i0["spec_issued"]
    assert i1["evals_cost"] == i0["evals_cost"]
    assert identity_holds(st0, i0) and identity_holds(st1, i1)


def test_both_forms_of_the_trial_gradient_step_agree(kin_round_runs):
    # the thread-per-agent blocks decide every speculation as the wave-per-agent step does
    for policy in (0, 1):
        Uw, _, stw, iw = kin_round_runs[False, policy]
        Uc, _, stc, ic = kin_round_runs[True, policy]
        assert torch.equal(Uw, Uc) and torch.equal(stw, stc)
        assert (iw["spec_issued"], iw["spec_used"]) == (ic["spec_issued"], ic["spec_used"])


def test_retry_policy_wastes_fewer_gradients(kin_round_runs):
    U1, _, st1, i1 = kin_round_runs[True, 1]
    U2, _, st2, i2 = kin_round_runs[True, 2]
    print({k: (i1[k], i2[k]) for k in ("rounds", "spec_issued", "spec_used", "evals_grad", "evals_cost")})
    assert torch.equal(U1, U2) and torch.equal(st1, st2)
    assert i2["spec_issued"] - i2["spec_used"] < i1["spec_issued"] - i1["spec_used"]
    assert i2["rounds"] >= i1["rounds"]
    assert identity_holds(st2, i2)
    # depth 2 (no speculation from the second doubling on) drops a subset of what depth 1 drops, and a dropped speculation
    # is never a wasted one: its waste lies between policy 1's and depth 1's
    Ud, _, std, idd = kin_round_runs[True, 22]
    print({k: idd[k] for k in ("rounds", "spec_issued", "spec_used")})
    assert torch.equal(U1, Ud) and torch.equal(st1, std) and identity_holds(std, idd)
    waste = lambda i: i["spec_issued"] - i["spec_used"]
    assert waste(i2) <= waste(idd) <= waste(i1)
    assert i2["spec_issued"] <= idd["spec_issued"] < i1["spec_issued"]


def test_chain_min_puts_the_thread_per_agent_blocks_into_the_launches(dev, monkeypatch):
    """The chain=True runs above mean something only if MPC_CHAIN_MIN=1 does put the blocks into the step launches.  A
    block leaves the agent it served in PH_W_LS_C with the launch's tag (phase word >= 64) until the next launch takes it;
    the wave-per-agent step never writes a tag.  A solve cut short by the round limit shows the records in between."""
    from model_predictive_control_amd import _lib
    N, x0 = 20, synthetic_states(0, 300, seed=5)
    cfg = mp.default_config(0, N, max_total_inner=600)
    tagged = {}
    for chain in (False, True):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("MPC_SOLO_MAX", "0")
        if chain:
            monkeypatch.setenv("MPC_CHAIN_MIN", "1")
        eng = mp.BatchedMPC(cfg, dev)
        eng.set_round_limit(40)
        with pytest.raises(_lib.MpcError, match="error -4"):
            eng.solve(T(x0, dev), T(straight_centerline(), dev), T(np.tile([1., 0.], (300, N)), dev))
        tagged[chain] = int((eng.debug_records(300)["phase"] >= 64).sum())
    print(tagged)
    assert tagged[False] == 0 and tagged[True] > 0


@pytest.mark.parametrize("model,N,B,kw,env", [
    (1, 12, 128, {}, {}),                                                     # Pacejka: the persistent kernel with the lookahead
    (0, 40, 200, dict(constr_mode=2, lane_halfwidth=0.05, Sigma0=10.0, max_total_inner=400, max_total_evals=2500),
     dict(MPC_SOLO_MAX=0)),                                                   # lane band, two elements per lane, round path
    (0, 20, 64, {}, dict(MPC_SOLO_ALL=4096)),                                 # the kinematic persistent kernel alone
], ids=["pacejka", "lane_band_n80", "solo_kinematic"])
def test_other_instantiations_keep_their_bits(dev, monkeypatch, model, N, B, kw, env):
    x0 = synthetic_states(model, B, seed=9)
    cfg = mp.default_config(model, N, **kw)
    Ud, ld, sd, idf = solve(monkeypatch, dev, cfg, x0, N, **env)
    U0, l0, s0, i0 = solve(monkeypatch, dev, cfg, x0, N, MPC_SPEC_POLICY=0, **env)
    print({k: (i0[k], idf[k]) for k in ("rounds", "spec_issued", "spec_used", "solo_agents")})
    assert torch.equal(Ud, U0) and torch.equal(sd, s0) and same(ld, l0)
    assert idf["spec_issued"] <= i0["spec_issued"]
    if "MPC_SOLO_MAX" not in env:
        assert idf["solo_agents"] == B and idf["rounds"] == 0
