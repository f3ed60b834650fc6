"""GPU tests of the solver state machine at options other than the reference's (tables, problems and oracle runs:
solver_options_common.py; their preconditions and the oracle's own behaviour at these values: test_solver_options_cpu.py;
measured figures: profiles/r27_solver_options.txt).

  a, b  PREFIX PARITY with the oracle: `max_total_inner = k` stops both implementations after k inner iterations, and the
        assertions are test_gpu_parity.test_iterate_prefix_parity's, the yardstick being the oracle against itself with
        its evaluations moved by 2 ulp: as many agents with the oracle's counts as the jittered oracle has (minus 2 %),
        status / outer / inner (and, with constraints, failed inner solves) equal where the evaluation counts are, median
        distance within 20x and largest within 100x the jittered oracle's -- controls, and multipliers where there are any;
  c     EVERY PATH THE SAME BITS at these options: rounds, persistent kernel, a hand-over between them, history from
        global memory / from a short LDS copy, no speculation, no lookahead;
  d     THE STALLING AGENT under limits on its retries: the oracle's counts exactly, the memo of failed retries changes
        nothing but the work, alone as inside a batch;
  e     THE RECORDS of the state machine held against the option values, without the oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import solver_options_common as S

pytestmark = pytest.mark.gpu

import model_predictive_control_amd as mp  # noqa: E402

SWITCHES = ("MPC_SPEC_POLICY", "MPC_SPEC_DEPTH", "MPC_CHAIN_MIN", "MPC_NO_CHAIN", "MPC_NO_SPEC", "MPC_SOLO_MAX", "MPC_SOLO_ALL",
            "MPC_LDS_PAIRS", "MPC_ALL_ROWS", "MPC_STEP_REGS", "MPC_NO_LOOKAHEAD", "MPC_NO_MEMO")
JITTER_SEED = (7,)                  # test_iterate_prefix_parity's
ids = lambda v: v if isinstance(v, str) else None


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)


def hip_solve(dev, prob, kw, k, solo_max=None, memo=None, x0=None):
    """(U, lam, statistics, last_solve_info, engine) of a fresh engine on a problem with an entry's options."""
    eng = mp.BatchedMPC(mp.default_config(prob["model"], prob["N"], **S.config_kw(prob, kw, k)), dev)
    if solo_max is not None:
        eng.set_solo_max(solo_max)
    if memo is not None:
        eng.set_memo(memo)
    x0 = prob["x0"] if x0 is None else x0
    U, lam, st = eng.solve(T(x0, dev), T(prob["cl"], dev), T(np.tile([1.0, 0.0], (x0.shape[0], prob["N"])), dev))
    return U, lam, st, eng.last_solve_info(), eng


def same_bits(a, b):
    """Controls, multipliers and all eight statistics columns."""
    return torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and ((a[1] is None and b[1] is None) or torch.equal(a[1], b[1]))


# ----------------------------------------------------------------------------- a, b: prefix parity
def _prefix_parity(dev, O, entry, pname, ks, constrained):
    prob, kw = S.problem(pname), S.options_of(entry)
    report, runs = [], []
    for k in ks:
        U, lam, st, _, _ = hip_solve(dev, prob, kw, k)
        U, st = U.cpu().numpy(), st.cpu().numpy()
        plain, (jit,) = S.reference_runs(O, kw, prob, k, JITTER_SEED)
        Uo, lo, so = plain
        same = st[:, 7] == so[:, 7]
        samej, dj = S.jitter_distances(plain, jit, 0)
        dh = np.abs(U - Uo).max(1)[same]
        row = [k, round(float(same.mean()), 4), round(float(samej.mean()), 4), "%.1e/%.1e" % (np.median(dh), dh.max()),
               "%.1e/%.1e" % (np.median(dj), dj.max())]
        lh = lj = None
        if constrained:
            lh = np.abs(lam.cpu().numpy() - lo).max(1)[same]
            lj = S.jitter_distances(plain, jit, 1)[1]
            row += ["%.1e/%.1e" % (np.median(lh), lh.max()), "%.1e/%.1e" % (np.median(lj), lj.max())]
        runs.append((k, st, so, same, samej, dh, dj, lh, lj))
        report.append(tuple(row))
    print("solver options prefix parity,", entry, "on", pname, "(k, equal-count fraction HIP vs oracle, jittered oracle vs oracle, "
          "median/max |dU| HIP, jittered" + (", median/max |dlam| HIP, jittered" if constrained else "") + "):", report)
    for k, st, so, same, samej, dh, dj, lh, lj in runs:
        assert same.mean() >= samej.mean() - 0.02, report
        assert (st[same, 2] == so[same, 2]).all() and (st[same, 1] == so[same, 1]).all() and (st[same, 0] == so[same, 0]).all(), report
        assert (st[:, 2] <= k).all() and (so[:, 2] <= k).all()
        assert np.median(dh) <= 20.0 * np.median(dj) + 1e-13 and dh.max() <= 100.0 * dj.max(), report
        if constrained:
            assert (st[same, 3] == so[same, 3]).all(), report
            assert np.median(lh) <= 20.0 * np.median(lj) + 1e-13 and lh.max() <= 100.0 * lj.max(), report


@pytest.mark.parametrize("entry,pname,ks", S.unconstrained_cases(), ids=ids)
def test_prefix_parity_unconstrained(dev, O, entry, pname, ks):
    _prefix_parity(dev, O, entry, pname, ks, constrained=False)
    prob, M = S.problem(pname), S.UNCONSTRAINED[entry].get("lbfgs_memory")
    if M is not None and pname in S.UNC_LARGE:
        # a memory below the pairs the step kernel's LDS plan would hold: the copy holds no more than the ring does
        P, lds, wps = C.c_int(), C.c_int(), C.c_int()
        from model_predictive_control_amd import _lib
        assert _lib.load().mpc_step_lds_plan(2 * prob["N"], M, 0, 1, 0, C.byref(P), C.byref(lds), C.byref(wps)) == 0
        assert 1 <= P.value <= M


@pytest.mark.parametrize("entry,pname,ks", S.alm_cases(), ids=ids)
def test_prefix_parity_alm(dev, O, entry, pname, ks):
    _prefix_parity(dev, O, entry, pname, ks, constrained=True)


# ----------------------------------------------------------------------------- c: every path, the same bits
def _paths(dev, monkeypatch, prob, kw, k, variants):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    rounds = hip_solve(dev, prob, kw, k, solo_max=0)
    assert rounds[3]["solo_agents"] == 0 and rounds[3]["rounds"] > 0
    solo = hip_solve(dev, prob, kw, k, solo_max=100000)
    assert solo[3]["solo_agents"] == prob["B"] and solo[3]["rounds"] == 0
    assert same_bits(solo, rounds)
    for name, env, solo_max in variants:
        for var, val in env.items():
            monkeypatch.setenv(var, val)
        run = hip_solve(dev, prob, kw, k, solo_max=solo_max)
        for var in env:
            monkeypatch.delenv(var)
        assert same_bits(run, rounds), name
        if "MPC_NO_SPEC" in env:
            assert run[3]["spec_issued"] == 0
        if "MPC_NO_LOOKAHEAD" in env:
            assert run[3]["lookahead_evals"] == 0
    return rounds, solo


@pytest.mark.parametrize("entry,pname,ks", S.unconstrained_cases() + S.alm_cases(), ids=ids)
def test_rounds_and_persistent_kernel_take_the_same_bits(dev, monkeypatch, entry, pname, ks):
    _paths(dev, monkeypatch, S.problem(pname), S.options_of(entry), max(ks), [])


VARIANT_CASES = [c for c in S.unconstrained_cases() if c[0] in ("combo", "tau1", "Lmax5") or c[:2] == ("mem1", "kin40")] + \
                [c for c in S.alm_cases() if c[:2] == ("maxit3_low", "lane")]


@pytest.mark.parametrize("entry,pname,ks", VARIANT_CASES, ids=ids)
def test_every_variant_takes_the_same_bits(dev, monkeypatch, entry, pname, ks):
    """History read from global memory (MPC_STEP_REGS), an LDS copy of three pairs (n > 64), no speculative gradients
    (statistics equal all the same, evaluation counts included), every speculative gradient issued (MPC_SPEC_POLICY=0),
    the persistent kernel without its lookahead, and a hand-over from the rounds to the persistent kernel in mid-solve."""
    prob = S.problem(pname)
    variants = []
    for solo_max in (0, 100000):
        variants += [("step_regs", {"MPC_STEP_REGS": "1"}, solo_max), ("no_spec", {"MPC_NO_SPEC": "1"}, solo_max),
                     ("spec_policy_0", {"MPC_SPEC_POLICY": "0"}, solo_max)]
    if 2 * prob["N"] > 64:
        variants.append(("lds_pairs_3", {"MPC_LDS_PAIRS": "3"}, 0))
    variants += [("no_lookahead", {"MPC_NO_LOOKAHEAD": "1"}, 100000), ("hand_over", {}, 8)]
    _paths(dev, monkeypatch, prob, S.options_of(entry), max(ks), variants)


# ----------------------------------------------------------------------------- d: the stalling agent
# Where the jittered oracle stays within ~1e-14 of the plain one (the path holds no amplifying step: every set whose
# jittered distance is below STALL_TIGHT), 100x that distance is less than two correct implementations of the model can
# be held to, and the bound is an absolute floor: four times the distance measured on the MI355X
# (profiles/r27_solver_options.txt), the convention of the closed-loop tests' STATE_BOUND.
STALL_TIGHT = 1e-13
STALL_FLOOR = {e: 6.7e-16 for e in ("outer8", "noprog2_outer8", "noprog30_outer8", "maxit15_outer8", "hess5_outer8")}   # measured 1.67e-16
STALL_FLOOR["Lmax1e8_inner400"] = 2.8e-14                                                                               # measured 6.94e-15


@pytest.mark.parametrize("entry", list(S.STALL))
def test_stalling_agent_under_retry_limits(dev, O, monkeypatch, entry):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    prob, (kw, _) = S.problem("stall"), S.STALL[entry]
    plain, jit = S.reference_runs(O, kw, prob, None, S.STALL_SEEDS)
    counts = plain[2][0, S.COUNTS]
    assert all(S.same_counts(j[2], plain[2]).all() for j in jit)           # (the precondition: test_solver_options_cpu.py)
    with_memo = hip_solve(dev, prob, kw, None, memo=True)
    without = hip_solve(dev, prob, kw, None, memo=False)
    st = with_memo[2].cpu().numpy()
    executed = [r[3]["evals_grad"] + r[3]["evals_cost"] for r in (with_memo, without)]
    dj = max(np.abs(j[0] - plain[0]).max() for j in jit)
    dh = np.abs(with_memo[0].cpu().numpy() - plain[0]).max()
    print("stalling agent,", entry, ": counts HIP", st[0, S.COUNTS].astype(int).tolist(), "oracle", counts.astype(int).tolist(),
          "; evaluations executed with / without the memo", executed, "; max |dU| HIP %.2e, jittered oracle %.2e" % (dh, dj))
    assert np.array_equal(st[0, S.COUNTS], counts)
    assert same_bits(with_memo, without)
    if counts[3] >= 2:
        assert executed[0] < executed[1], executed
    # inside a batch on the round path: the same bits as alone
    X = S.synthetic_states(1, 200, seed=11)
    X[37] = prob["x0"][0]
    Ub, _, sb, info, _ = hip_solve(dev, prob, kw, None, solo_max=0, x0=X)
    assert info["solo_agents"] == 0 and torch.equal(Ub[37], with_memo[0][0]) and torch.equal(sb[37], with_memo[2][0])
    assert dh <= (STALL_FLOOR[entry] if dj < STALL_TIGHT else 100.0 * dj), (dh, dj)


# ----------------------------------------------------------------------------- e: the records against the options
@pytest.mark.parametrize("pname", S.UNC_SMALL)
@pytest.mark.parametrize("entry", ["combo", "Lmax5", "Lmin50"])
def test_records_honour_the_options(dev, monkeypatch, entry, pname):
    """mpc_debug_records after twelve iterations (names: mpc_debug_record_names, in the order of mpc_solver.hpp's record
    enum): L and Ln (the estimate at the iterate and at the accepted trial) inside [L_min, L_max], gamma = Lgamma_factor / L
    for both (one division, then exact halvings: 2 ulp), the L-BFGS ring inside its memory, and the accepted line-search step
    -- the record holds it halved, as PH_W_LS_C leaves `tau` -- zero or in [tau_min, 1].  On both paths."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    prob, kw = S.problem(pname), S.UNCONSTRAINED[entry]
    cfg = mp.default_config(prob["model"], prob["N"], **S.config_kw(prob, kw, 12))
    for solo_max in (0, 100000):
        _, _, st, _, eng = hip_solve(dev, prob, kw, 12, solo_max=solo_max)
        rec = eng.debug_records(prob["B"])
        assert np.array_equal(rec["inner_tot"], st[:, 2].cpu().numpy()) and (rec["inner_tot"] == 12).mean() >= 0.9
        for L, gamma in ((rec["L"], rec["gamma"]), (rec["Ln"], rec["gamman"])):
            assert (L >= cfg.L_min).all() and (L <= cfg.L_max).all()
            assert (np.abs(gamma * L / cfg.Lgamma_factor - 1.0) <= 4 * np.finfo(float).eps).all()
        fill = np.where(rec["lfull"] != 0, cfg.lbfgs_memory, rec["lidx"])
        assert (rec["lidx"] >= 0).all() and (rec["lidx"] < cfg.lbfgs_memory).all() and (fill <= cfg.lbfgs_memory).all()
        tau = 2.0 * rec["tau"]
        assert ((tau == 0) | ((tau >= cfg.tau_min) & (tau <= 1.0))).all()
        # the options are what made these records: the bound each entry sets is reached
        if entry == "combo":
            assert fill.max() == cfg.lbfgs_memory and (rec["k"] <= cfg.max_iter).all()
        if entry == "Lmin50":
            assert (rec["L"] == cfg.L_min).any()
        if entry == "Lmax5":
            assert (2.0 * rec["L"] > cfg.L_max).any()
