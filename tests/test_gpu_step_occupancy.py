"""GPU test: the step kernel's launch shape -- agents per workgroup (MPC_APB) and the pairs of the L-BFGS history its
LDS copy holds (MPC_LDS_PAIRS) -- changes nothing but the time.  The benchmark's problem at 16 384 agents in one
sub-batch group (the shape of one of the headline's four group launches, where the default takes 32 agents per
workgroup) and in the default grouping, kinematic N = 20 and Pacejka N = 12: controls, multipliers and the eight
statistics columns are equal bit for bit across every combination."""
import numpy as np
import pytest
import torch

from conftest import straight_centerline

import model_predictive_control_amd as mp

pytestmark = pytest.mark.gpu

B = 16384
SWITCHES = ("MPC_APB", "MPC_LDS_PAIRS", "MPC_GROUPS", "MPC_SOLO_MAX")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.mark.parametrize("model, N", [(mp.MODEL_KINEMATIC, 20), (mp.MODEL_PACEJKA, 12)])
def test_launch_shape_changes_no_bits(dev, monkeypatch, model, N):
    import bench
    X0 = torch.tensor(bench.synthetic_states(model, 0, B), dtype=torch.float64, device=dev)
    cl = torch.tensor(straight_centerline(), dtype=torch.float64, device=dev)
    U0 = torch.tensor([1.0, 0.0], dtype=torch.float64, device=dev).repeat(B, N)
    cfg = mp.default_config(model, N)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)

    def run(**env):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        eng = mp.BatchedMPC(cfg, dev)
        U, lam, st = eng.solve(X0, cl, U0)
        rounds = eng.last_solve_info()["rounds"]
        return U, lam, st, rounds

    U, lam, st, rounds = run()                                # default grouping
    assert rounds > 0 and st.shape == (B, mp.NSTATS)
    assert (st[:, 0] == 1).all()
    variants = [dict(MPC_GROUPS=1)]
    variants += [dict(MPC_GROUPS=1, MPC_APB=apb, **pairs) for apb in (64, 32, 16) for pairs in ({}, dict(MPC_LDS_PAIRS=3))]
    for env in variants:
        U2, lam2, st2, rounds2 = run(**env)
        assert rounds2 > 0, env
        assert torch.equal(U2, U), env
        assert torch.equal(st2, st), env
        assert (lam is None) == (lam2 is None), env
        if lam is not None:
            assert torch.equal(lam2, lam), env
    monkeypatch.delenv("MPC_GROUPS", raising=False)
    monkeypatch.delenv("MPC_APB", raising=False)
    monkeypatch.delenv("MPC_LDS_PAIRS", raising=False)
    assert np.isfinite(U.cpu().numpy()).all()
