"""CPU tests behind test_gpu_solver_options.py (solver options other than the reference's; tables and problems in
solver_options_common.py).  Two things, both on the oracle alone:

  * the PRECONDITIONS of the GPU tests: every option set changes what the solver does inside the prefix it is run at
    (bite), the oracle takes the same decisions there with its evaluations moved by 2 ulp (stability), and the stalling
    agent walks the recorded path under five jitter seeds.  They are conditions on the inputs: an entry that stops
    meeting them is replaced by another value, the bars stay;
  * the oracle HONOURS the options: it is the reference of the GPU tests and nothing else runs it at these values.  Its
    per-iteration and per-outer-iteration traces are held against the option values themselves."""
import ctypes as C

import numpy as np
import pytest

import solver_options_common as S

UNC_BITE, ALM_BITE, STABLE = 0.5, 0.3, 0.95
AGENTS = 8


# ----------------------------------------------------------------------------- preconditions
@pytest.mark.parametrize("entry,pname,ks", S.unconstrained_cases(), ids=lambda v: v if isinstance(v, str) else None)
def test_unconstrained_entry_bites_and_is_stable(O, entry, pname, ks):
    prob, kw = S.problem(pname), S.UNCONSTRAINED[entry]
    assert S.bite(O, kw, prob, max(ks)) >= UNC_BITE
    for k in ks:
        assert S.stability(O, kw, prob, k) >= STABLE, k


@pytest.mark.parametrize("entry", list(S.ALM))
def test_alm_entry_bites_and_is_stable(O, entry):
    kw, probs, _ = S.ALM[entry]
    assert max(S.alm_bite(O, entry, S.problem(p), 25) for p in probs) >= ALM_BITE
    for p in probs:
        for k in S.alm_ks(entry):
            assert S.stability(O, kw, S.problem(p), k) >= STABLE, (p, k)


def test_the_tables_hold_what_they_promise():
    """Sixteen, eleven and eleven option sets, the larger shapes for the six sets that also run on the
    two-elements-per-lane kernel, and option names that exist."""
    assert len(S.UNCONSTRAINED) == 16 and len(S.ALM) == 11 and len(S.STALL) == 11
    assert {p for _, p, _ in S.unconstrained_cases()} == {"kin8", "pac6", "kin20", "kin40"}
    assert {e for e, p, _ in S.unconstrained_cases() if p == "kin40"} == set(S.UNC_ALSO_LARGE)
    from oracle import oracle
    fields = {f[0] for f in oracle.OrcConfig._fields_}
    for e in list(S.UNCONSTRAINED) + list(S.ALM) + list(S.STALL):
        assert set(S.options_of(e)) <= fields, e


@pytest.mark.parametrize("entry", list(S.STALL))
def test_stalling_agent_walks_its_recorded_path(O, entry):
    kw, counts = S.STALL[entry]
    plain, jit = S.reference_runs(O, kw, S.problem("stall"), None, S.STALL_SEEDS)
    assert tuple(int(v) for v in plain[2][0, S.COUNTS]) == counts
    for j in jit:
        assert S.same_counts(j[2], plain[2]).all()


# ----------------------------------------------------------------------------- the oracle honours the options
def _traces(O, prob, kw, k, agents=AGENTS):
    """[(statistics, per-iteration trace, per-outer-iteration trace)] of the first agents of a problem."""
    cfg = O.default_config(prob["model"], prob["N"], **S.config_kw(prob, kw, k))
    out = []
    for a in range(min(agents, prob["B"])):
        _, _, st, it = O.solve_itertrace(cfg, prob["x0"][a], prob["cl"], prob["U0"][a])
        _, _, st2, tr = O.solve_traced(cfg, prob["x0"][a], prob["cl"], prob["U0"][a], max_rows=512)
        assert np.array_equal(st, st2) and len(it) == st[2] and len(tr) == st[1]
        out.append((st, it, tr))
    return cfg, out


def _backtracks(tr):
    """(backtracked while still at the first penalty, backtracked later): orc_solve's init_red and pen_red."""
    first, init_red, pen_red = True, 0, 0
    for row in tr:
        if row[8]:
            init_red, pen_red = init_red + first, pen_red + (not first)
        else:
            first = False
    return init_red, pen_red


def _check_traces(cfg, runs):
    """What every trace must show, whatever the option values.  Columns: oracle.ITRACE_COLS / oracle.TRACE_COLS."""
    for st, it, tr in runs:
        # inner solve: the row of iteration k (0-based) holds k + 1; an inner solve stops AT k == max_iter
        assert (it[:, 2] >= 1).all() and (it[:, 2] <= cfg.max_iter).all()
        assert (it[:, 9] <= cfg.lbfgs_memory).all() and (it[:, 9] >= 0).all()
        assert (it[:, 6] >= cfg.L_min).all() and (it[:, 6] <= cfg.L_max).all()
        assert np.array_equal(it[:, 7], cfg.Lgamma_factor / it[:, 6])            # gamma = Lgamma_factor / L (x 2^j: exact)
        tau = np.abs(it[:, 4])                                                   # (a safe prox step is reported negative)
        assert ((tau == 0) | ((tau >= cfg.tau_min) & (tau <= 1.0))).all()
        # outer loop
        assert st[1] <= cfg.max_outer and (st[2] <= cfg.max_total_inner)
        if len(tr) and np.isfinite(tr[:, 7]).all():
            assert (tr[:, 7] <= cfg.Sigma_max).all()
        # the tolerance schedule: eps0, times rho after an inner solve whose result is kept, floored at alm_eps;
        # after one that is backtracked over, eps0_increase (still at the first penalty) or a slower rho
        eps, eps_old, rho, first = cfg.eps0, np.nan, cfg.rho, True
        for row in tr:
            assert row[1] == eps, (row, eps)
            if row[8]:
                if first:
                    eps *= cfg.eps0_increase
                else:
                    rho = min(0.5, rho * cfg.rho_increase)
                    eps = max(rho * eps_old, cfg.alm_eps)
            else:
                eps_old, eps, first = eps, max(rho * eps, cfg.alm_eps), False
        # retries (orc_solve): a failed inner solve is backtracked over -- its iterate dropped, tolerance and penalty
        # changed, counted in init_red while the first penalty stands and in pen_red after -- unless its result is kept
        # (overwrite): the last outer iteration, the last the budget allows, or the retries are used up
        # (init_red == max_num_initial_retries, pen_red == max_num_retries, their sum == max_total_num_retries).  So
        # backtracks never exceed the limits, and every other failure is a kept one:
        #     failures = backtracks + kept failures,    backtracks <= the limits.
        # (With the limits reached every later inner solve is kept, failed or not: max_num_retries = 3 shows 3 + 1.)
        init_red, pen_red = _backtracks(tr)
        assert init_red <= cfg.max_num_initial_retries and pen_red <= cfg.max_num_retries
        assert init_red + pen_red <= cfg.max_total_num_retries
        failed = tr[:, 2] != 1
        assert (failed | (tr[:, 8] == 0)).all()                                  # only a failed inner solve is backtracked over
        kept = failed & (tr[:, 8] == 0)
        kept_failures = int(kept.sum())
        assert (tr[kept, 9] == 1).all() or (st[0] == 2 and (tr[kept, 9] == 1)[:-1].all())   # overwrite, or out of budget at the end
        assert st[3] == init_red + pen_red + kept_failures


@pytest.mark.parametrize("entry,pname,ks", [c for c in S.unconstrained_cases() if c[1] in S.UNC_SMALL] + S.alm_cases(),
                         ids=lambda v: v if isinstance(v, str) else None)
def test_oracle_honours_the_options_on_prefixes(O, entry, pname, ks):
    prob = S.problem(pname)
    cfg, runs = _traces(O, prob, S.options_of(entry), max(ks))
    for name, v in S.options_of(entry).items():
        assert getattr(cfg, name) == v
    _check_traces(cfg, runs)
    it = np.concatenate([r[1] for r in runs])
    if entry in ("tau1", "tau_half"):                     # never a step strictly between 0 and tau_min
        assert set(np.abs(it[:, 4]).tolist()) <= ({0.0, 1.0} if entry == "tau1" else {0.0, 0.5, 1.0})
        assert (np.abs(it[:, 4]) == 1.0).any()
    if entry in ("mem1", "mem3", "combo"):                # ... and the bound is reached
        assert it[:, 9].max() == cfg.lbfgs_memory
    if entry == "Lmin50":
        assert (it[:, 6] == cfg.L_min).any()
    if entry in ("Lmax1", "Lmax5"):                       # (a doubling needs 2 L <= L_max: the cap shows as estimates it stopped)
        assert (2.0 * it[:, 6] > cfg.L_max).any()
    if entry.startswith("maxit"):
        assert it[:, 2].max() == cfg.max_iter


@pytest.mark.parametrize("pname", S.UNC_SMALL)
def test_oracle_step_size_heuristic_costs_evaluations(O, pname):
    """hess_heuristic = 1 (a finite-difference Hessian-vector product at the top of every iteration after the first)
    against hess_heuristic = 0 (never): more evaluations per inner iteration, for every agent."""
    prob = S.problem(pname)
    (_, _, s1), _ = S.reference_runs(O, dict(hess_heuristic=1), prob, 12, ())
    (_, _, s0), _ = S.reference_runs(O, dict(hess_heuristic=0), prob, 12, ())
    assert (s1[:AGENTS, 2] == 12).all() and (s0[:AGENTS, 2] == 12).all()
    assert (s1[:AGENTS, 7] / s1[:AGENTS, 2] > s0[:AGENTS, 7] / s0[:AGENTS, 2]).all()


@pytest.mark.parametrize("entry", list(S.STALL))
def test_oracle_honours_the_options_on_the_stalling_agent(O, entry):
    kw, counts = S.STALL[entry]
    cfg, runs = _traces(O, S.problem("stall"), kw, None)
    _check_traces(cfg, runs)
    st, it, tr = runs[0]
    assert tuple(int(v) for v in st[S.COUNTS]) == counts
    init_red, pen_red = _backtracks(tr)
    if entry == "retr3_outer6":
        assert (pen_red, int(st[3])) == (3, 3 + 1)        # the three retries, and the kept failure after them
    if entry == "tot5_outer8":
        assert (init_red + pen_red, int(st[3])) == (5, 5 + 1)
    if entry == "retr0_outer3":
        assert (init_red + pen_red, int(st[3])) == (0, 1)
    if entry.startswith("noprog"):                        # NoProgress (5) after more than max_no_progress idle iterations
        assert (tr[:, 2] == 5).any() and (tr[tr[:, 2] == 5, 3] > cfg.max_no_progress).all()
    if entry == "evals500":
        assert st[0] == 2 and st[7] >= cfg.max_total_evals and tr[-2, 10] < cfg.max_total_evals


def test_step_lds_plan_holds_no_more_pairs_than_the_memory():
    """The step kernel's LDS copy of the L-BFGS history at memories below what the plan would allow (twelve pairs at
    n = 40, fewer at n = 80): never more pairs than the ring has."""
    from model_predictive_control_amd import _lib
    _lib.build()
    L = _lib.load()
    for n in (40, 80):
        for M in (1, 2, 3):
            P, lds, wps = C.c_int(), C.c_int(), C.c_int()
            assert L.mpc_step_lds_plan(n, M, 0, 1, 0, C.byref(P), C.byref(lds), C.byref(wps)) == 0
            assert 1 <= P.value <= M
