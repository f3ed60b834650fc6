"""CPU tests of the keep-out discs (constr_mode CONSTR_DISCS, mpc_set_agent_discs): the checker of
tests/discs_common.py against itself (its exact gradient against central differences of its own psi), the host-side
pieces of the feature that need no GPU (row layout, m, the default row, the configuration check), and the recorded
reference solves of tests/golden/discs_reference.npz re-derived in part."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

import discs_common as D
import model_predictive_control_amd as mp
from model_predictive_control_amd import _lib


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.load()


@pytest.mark.parametrize("name", list(D.SCENES))
def test_checker_gradient_against_central_differences(O, name):
    """the VJP route through the oracle's STATE_SQ mode is the gradient of the numpy psi: within the project's
    finite-difference bar of 1e-6 ||grad psi||, with discs active (y < 0 and violated discs both occur)"""
    model, N, x0, scene = D.SCENES[name]
    cfgs = D.configs(O, model, N)
    cl = D.line_centerline()
    rng = np.random.default_rng(1)
    U = np.tile([0.6, 0.02], N) + rng.uniform(-.05, .05, 2 * N)
    y = rng.uniform(-1, 0.2, 2 * N)
    Sig = 10 ** rng.uniform(0, 3, 2 * N)
    psi, yhat, grad, g = D.psi_yhat(O, cfgs, x0, cl, U, scene(N), y, Sig)
    assert (yhat < 0).sum() >= 5 and (yhat == 0).sum() >= 5
    fd = D.psi_fd_grad(O, cfgs, x0, cl, U, scene(N), y, Sig)
    assert np.abs(grad - fd).max() <= 1e-6 * np.linalg.norm(grad)
    # no disc active: psi is f and the gradient the oracle's own
    p0, yh0, g0, _ = D.psi_yhat(O, cfgs, x0, cl, U, np.zeros((N, 2, 3)), np.zeros(2 * N), Sig)
    f, gf = O.psi(cfgs[0], x0, cl, U)
    assert p0 == f and not yh0.any() and np.abs(g0 - gf).max() <= 1e-13 * np.linalg.norm(gf)


def test_disc_rows_layout():
    cfg = mp.default_config(mp.MODEL_KINEMATIC, 5, constr_mode=mp.CONSTR_DISCS)
    N, P = 5, 3
    assert _lib.disc_row_width(cfg) == 3 * mp.NDISC * N == 30
    z = mp.disc_rows(cfg, P)
    assert z.shape == (P, 30) and z.dtype == np.float64 and not z.any()
    rng = np.random.default_rng(0)
    c, r = rng.normal(size=(P, N, 2, 2)), rng.uniform(0, 1, (P, N, 2))
    t = mp.disc_rows(cfg, P, centres=c, radii=r)
    for p in range(P):
        for k in range(N):
            for j in range(2):
                e = t[p, (k * 2 + j) * 3:(k * 2 + j) * 3 + 3]          # [N][NDISC][3] = (cx, cy, r)
                assert e[0] == c[p, k, j, 0] and e[1] == c[p, k, j, 1] and e[2] == r[p, k, j]
    # every-row forms
    t1 = mp.disc_rows(cfg, P, centres=c[0], radii=r[0])
    assert all(np.array_equal(t1[p], t[0]) for p in range(P))
    assert np.array_equal(mp.disc_rows(cfg, P, radii=0.25).reshape(P, N, 2, 3)[..., 2], np.full((P, N, 2), 0.25))
    with pytest.raises(ValueError):
        mp.disc_rows(cfg, P, centres=c[:, :4])
    with pytest.raises(ValueError):
        mp.disc_rows(cfg, P, radii=r[:2])
    with pytest.raises(ValueError):
        mp.disc_rows(cfg, 0)


@pytest.mark.parametrize("model,N", [(0, 20), (1, 12), (0, 1), (1, 64)])
def test_m_is_two_per_stage_and_the_default_row_is_zeros(L, model, N):
    cfg = mp.default_config(model, N, constr_mode=mp.CONSTR_DISCS)
    assert L.mpc_m(C.byref(cfg)) == 2 * N
    row = (C.c_double * (6 * N + 1))(*([7.0] * (6 * N + 1)))
    assert L.mpc_default_discs(C.byref(cfg), row) == 0
    assert list(row[:6 * N]) == [0.0] * (6 * N) and row[6 * N] == 7.0      # MPC_DISC_ROW(N) doubles, no more
    assert np.array_equal(mp.default_discs(cfg), np.zeros(6 * N))
    assert L.mpc_default_discs(None, row) == -1 and L.mpc_default_discs(C.byref(cfg), None) == -1


def test_mode_is_accepted_and_the_next_one_is_not(L):
    """mpc_create checks the configuration before it touches the device: CONSTR_DISCS passes the check (and then fails on
    the missing device, or succeeds), constr_mode 4 does not"""
    h = C.c_void_p()
    cfg = mp.default_config(mp.MODEL_KINEMATIC, 20, constr_mode=mp.CONSTR_DISCS)
    rc = L.mpc_create(C.byref(cfg), 0, C.byref(h))
    if rc == 0:
        L.mpc_destroy(h)
    else:
        assert b"constr_mode" not in L.mpc_last_error()
    cfg = mp.default_config(mp.MODEL_KINEMATIC, 20, constr_mode=4)
    assert L.mpc_create(C.byref(cfg), 0, C.byref(h)) == -1 and b"constr_mode" in L.mpc_last_error()


def test_header_constants_and_mirror_agree():
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "mpc_hip.h")).read()
    assert "MPC_CONSTR_DISCS = 3" in hdr and "#define MPC_NDISC 2" in hdr and "#define MPC_DISC_ROW(N) (3 * MPC_NDISC * (N))" in hdr
    assert (mp.CONSTR_DISCS, mp.NDISC, D.NDISC) == (3, 2, 2)
    for name in ("mpc_default_discs", "mpc_set_agent_discs", "mpc_discs_from_plans"):
        assert name in _lib.EXPORTS and name in hdr


def test_recorded_reference_solves_are_what_the_checker_gives(O):
    """tests/golden/discs_reference.npz holds what reference_solve returns (tests/golden/make_discs_golden.py): one entry
    of the Pacejka scene (the quickest) is solved again; all entries are feasible stationary points by the checker"""
    ref = np.load(os.path.join(GOLDEN, "discs_reference.npz"))
    shifts = D.scene_shifts()
    assert np.array_equal(ref["shifts"], shifts)
    model, N, x0, scene = D.SCENES["pacejka"]
    U, lam, _ = D.reference_solve(O, D.configs(O, model, N), x0, D.line_centerline(), scene(N, shifts[3]))
    assert np.abs(U - ref["U_pacejka"][3]).max() <= 1e-6 and np.abs(lam - ref["lam_pacejka"][3]).max() <= 1e-4
    for name, (model, N, x0, scene) in D.SCENES.items():
        cfgs = D.configs(O, model, N)
        for p in range(D.NSHIFT):
            U, lam = ref["U_" + name][p], ref["lam_" + name][p]
            g = D.disc_g(O.rollout(cfgs[0], x0, U), scene(N, shifts[p]))[0]
            assert g.min() >= -1e-7 and (lam <= 0).all() and 1 <= (lam < 0).sum() <= 6
            assert np.abs(g[lam < 0]).max() <= 1e-7
