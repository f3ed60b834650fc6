"""Solver options other than the reference's: the option sets, the problems and the oracle runs that
test_solver_options_cpu.py and test_gpu_solver_options.py share.

`mpc_config` steers the solver state machine with about thirty fields (inner solve, ALM outer loop, retries); the rest
of the suite runs it at the reference's values.  Here it runs at other values, on SHORT PREFIXES (`max_total_inner = k`:
the first k inner iterations of the long solve, see test_gpu_parity.test_iterate_prefix_parity) at which the CPU oracle
is insensitive to 2 ulp of evaluation noise, and on one agent whose inner solves stall.  Three tables:

  UNCONSTRAINED  options of the inner solve, on unconstrained problems, k = 3, 6, 12;
  ALM            options of the outer loop and of its retries, on the two feasible constrained problems of
                 test_gpu_parity.test_persistent_kernel_is_bit_identical, k = 10, 25 (60 with max_iter = 3);
  STALL          options that bound the retries of the Pacejka benchmark's stalling agent, with the oracle's
                 (status, outer, inner, failures, evaluations) for each.

An entry is usable only where it BITES (the option changes what the solver does within k iterations) and where the
oracle is STABLE (the same counts with its evaluations moved by 2 ulp): test_solver_options_cpu.py asserts both, and

    python tests/solver_options_common.py

prints the figures for every entry (profiles/r27_solver_options.txt holds a copy)."""
import numpy as np

from conftest import straight_centerline, synthetic_states

COUNTS = [0, 1, 2, 3, 7]            # statistics columns: status, outer, inner, failed inner solves, evaluations
JITTER_ULPS = 2                     # the HIP transcendentals are within 2 ulp of libm (test_device_math)
SEEDS = (7, 8)                      # jitter seeds of the stability figures
STALL_SEEDS = (1, 2, 3, 4, 5)
BITE_DU = 1e-6

# ----------------------------------------------------------------------------- problems
# name -> (model, N, B, seed)
_SHAPES = {"kin8": (0, 8, 64, 3), "pac6": (1, 6, 64, 3), "kin20": (0, 20, 32, 3), "kin40": (0, 40, 32, 3), "pac20": (1, 20, 32, 3),
           "lane": (0, 12, 64, 17), "squares": (1, 10, 64, 17), "stall": (1, 12, 1, 0)}
_PROBLEMS = {}


def problem(name):
    """{model, N, B, x0, U0, cl, base}: `base` holds the options that make the problem (constraints), to which an
    entry's options are added."""
    if name not in _PROBLEMS:
        model, N, B, seed = _SHAPES[name]
        base = {}
        if name == "stall":
            import bench
            x0 = bench.synthetic_states(1, 48296, 48297)      # test_failed_retries_are_replayed_not_recomputed's agent
        else:
            x0 = synthetic_states(model, B, seed=seed)
        if name == "lane":
            x0[:, 1] = np.clip(x0[:, 1], -0.04, 0.04)
            base = dict(constr_mode=2, lane_halfwidth=0.05, Sigma0=10.0)
        if name == "squares":
            x0[:, 0] *= 3.9 / 5.0
            x0[:, 3] = np.minimum(x0[:, 3], 0.65)
            base = dict(constr_mode=1, D_lb=[-np.inf] * 6, D_ub=[0.0] * 6, g_off=[20, 1, 1, 0.5, 1, 0.1], Sigma0=10.0)
        _PROBLEMS[name] = dict(name=name, model=model, N=N, B=B, x0=x0, U0=np.tile([1.0, 0.0], (B, N)), cl=straight_centerline(),
                               base=base)
    return _PROBLEMS[name]


def config_kw(prob, cfg_kw, k=None):
    """The keyword arguments of default_config (the oracle's and the library's alike) for an entry on a problem."""
    kw = dict(prob["base"])
    kw.update(cfg_kw)
    if k is not None:
        kw["max_total_inner"] = k
    return kw


# ----------------------------------------------------------------------------- the three tables
UNC_KS = (3, 6, 12)
UNC_SMALL = ("kin8", "pac6")
UNC_LARGE = ("kin20", "kin40")       # n = 40: one element per lane; n = 80: two elements per lane, capped LDS history
UNCONSTRAINED = {
    "mem1": dict(lbfgs_memory=1), "mem3": dict(lbfgs_memory=3),
    "hess1": dict(hess_heuristic=1), "hess4": dict(hess_heuristic=4),
    "tau1": dict(tau_min=1.0), "tau_half": dict(tau_min=0.5),
    "maxit1": dict(max_iter=1), "maxit4": dict(max_iter=4),
    "Lmin50": dict(L_min=50.0),
    "Lmax1": dict(L_max=1.0), "Lmax5": dict(L_max=5.0),
    "Lgam": dict(Lgamma_factor=0.5),
    "lip": dict(lip_eps=1e-4, lip_delta=1e-8),
    "qub": dict(qub_tol=1e-3),
    "eps0": dict(eps0=1e-2, rho=0.5),
    "combo": dict(lbfgs_memory=2, hess_heuristic=3, tau_min=0.25, Lgamma_factor=0.7, max_iter=5),
}
UNC_ALSO_LARGE = ("mem1", "mem3", "combo", "hess1", "tau1", "Lmax5")


def unconstrained_cases():
    """[(entry, problem, ks)] of the GPU prefix test.  With L_max = 5 the oracle's own counts stop being stable under
    jitter at N >= 20 (every descent-lemma test sits against the cap: 0.88 of the agents at N = 20 by k = 12, 0.84 at
    N = 40 by k = 6): those two cases stop at k = 6 and at k = 3."""
    out = [(e, p, UNC_KS) for e in UNCONSTRAINED for p in UNC_SMALL]
    out += [(e, p, {"kin20": (3, 6), "kin40": (3,)}[p] if e == "Lmax5" else UNC_KS) for e in UNC_ALSO_LARGE for p in UNC_LARGE]
    return out


ALM_KS = (10, 25)
ALM = {     # entry -> (options, the problems it runs on, the entry its bite is measured against: None = the reference's values)
    "Delta3": (dict(Delta=3.0), ("lane", "squares"), None),
    "Sig1": (dict(Sigma0=1.0), ("lane", "squares"), None),
    "Sig1e3": (dict(Sigma0=1e3), ("lane", "squares"), None),
    "eps0.1": (dict(eps0=0.1), ("lane", "squares"), None),
    # (lane band: the oracle keeps its counts under jitter for 0.91 of the agents only at k = 25)
    "rho.5": (dict(rho=0.5), ("squares",), None),
    # theta alone (0.02 ... 2) changes at most 0.22 of the agents by k = 25, Sigma_max = 100 0.14: theta with the
    # slower tolerance schedule (more penalty updates inside 25 iterations), and a cap of twice Sigma0
    "rho.5_theta.9": (dict(rho=0.5, theta=0.9), ("squares",), "rho.5"),
    "Sigmax20": (dict(Sigma_max=20.0), ("lane", "squares"), None),
    "maxit3": (dict(max_iter=3), ("lane", "squares"), None),
    "maxit3_low": (dict(max_iter=3, Delta_lower=0.5, Sigma0_lower=0.3, eps0_increase=3.0, rho_increase=1.5), ("lane", "squares"),
                   "maxit3"),
    "maxit3_retr1": (dict(max_iter=3, max_num_retries=1, max_num_initial_retries=1), ("lane", "squares"), "maxit3"),
    "maxit3_tot2": (dict(max_iter=3, max_total_num_retries=2), ("lane", "squares"), "maxit3"),
}
ALM_K60 = ("maxit3", "maxit3_low")


def alm_bite(O, entry, prob, k):
    kw, _, against = ALM[entry]
    return bite(O, kw, prob, k, against=ALM[against][0] if against else None)


def alm_ks(entry):
    """k = 60 only where the oracle is still stable there: inner solves that end after three iterations, with the
    reference's retry limits (with max_num_retries = 1 or max_total_num_retries = 2 it is stable for 0.72 - 0.95)."""
    return ALM_KS + ((60,) if entry in ALM_K60 else ())


def alm_cases():
    """[(entry, problem, ks)] of the GPU prefix test.  Sigma0 = 1e3 on the state squares stops at k = 10: by k = 25 four
    agents (10, 37, 55, 56) take decisions whose margins in the oracle (1e-5 .. 1e-4) are within the drift of 4e-6 .. 7e-4
    accumulated by then; the jittered oracle flips two to four of the same agents under every one of twenty seeds
    (profiles/r27_solver_options.txt)."""
    return [(e, p, (10,) if (e, p) == ("Sig1e3", "squares") else alm_ks(e)) for e, (_, probs, _) in ALM.items() for p in probs]


STALL = {   # entry -> (options, the oracle's (status, outer, inner, failures, evaluations))
    "outer8": (dict(max_outer=8), (3, 8, 149, 7, 855)),
    "retr3_outer6": (dict(max_num_retries=3, max_outer=6), (3, 6, 102, 4, 595)),
    "retr0_outer3": (dict(max_num_retries=0, max_outer=3), (3, 3, 67, 1, 330)),
    "tot5_outer8": (dict(max_total_num_retries=5, max_outer=8), (3, 8, 144, 6, 835)),
    "noprog2_outer8": (dict(max_no_progress=2, max_outer=8), (3, 8, 65, 7, 680)),
    "noprog30_outer8": (dict(max_no_progress=30, max_outer=8), (3, 8, 429, 7, 1436)),
    "maxit15_outer8": (dict(max_iter=15, max_outer=8), (3, 8, 107, 7, 771)),
    "hess5_outer8": (dict(hess_heuristic=5, max_outer=8), (3, 8, 149, 7, 876)),
    "Lmax1e8_inner400": (dict(L_max=1e8, max_total_inner=400), (2, 2, 400, 1, 2053)),
    "tau1_inner300": (dict(tau_min=1.0, max_total_inner=300), (2, 3, 300, 1, 971)),
    "evals500": (dict(max_total_evals=500), (2, 6, 87, 5, 504)),
}


def options_of(entry):
    if entry in UNCONSTRAINED:
        return UNCONSTRAINED[entry]
    return (ALM[entry] if entry in ALM else STALL[entry])[0]


# ----------------------------------------------------------------------------- oracle runs
_RUNS = {}


def _key(v):
    return tuple(_key(x) for x in v) if isinstance(v, (list, tuple)) else v


def reference_runs(O, cfg_kw, prob, k, seeds):
    """(plain, [jittered per seed]): each (U, lam, statistics) of the oracle on `prob` with `cfg_kw` and the inner
    iteration budget k (None: the configuration's own).  Computed once per argument set; the arrays are shared, so a
    caller leaves them unchanged."""
    key = (prob["name"], tuple(sorted((n, _key(v)) for n, v in cfg_kw.items())), k)
    cfg = O.default_config(prob["model"], prob["N"], **config_kw(prob, cfg_kw, k))
    nthreads = 1 if prob["B"] == 1 else 0

    def run(seed):
        if key + (seed,) not in _RUNS:
            if seed is None:
                r = O.solve_batch(cfg, prob["x0"], prob["cl"], prob["U0"], nthreads=nthreads)
            else:
                with O.eval_jitter(JITTER_ULPS, seed):
                    r = O.solve_batch(cfg, prob["x0"], prob["cl"], prob["U0"], nthreads=nthreads)
            for a in r:
                a.setflags(write=False)
            _RUNS[key + (seed,)] = r
        return _RUNS[key + (seed,)]

    return run(None), [run(seed) for seed in seeds]


def same_counts(sa, sb):
    """Per agent: the same (status, outer, inner, failures, evaluations)."""
    return (sa[:, COUNTS] == sb[:, COUNTS]).all(1)


def stability(O, cfg_kw, prob, k, seeds=SEEDS):
    """The smallest fraction, over the seeds, of agents on which the jittered oracle takes the plain oracle's counts."""
    plain, jit = reference_runs(O, cfg_kw, prob, k, seeds)
    return min(float(same_counts(j[2], plain[2]).mean()) for j in jit)


def bite(O, cfg_kw, prob, k, against=None):
    """The fraction of agents on which the options change the first k iterations against the reference's values (or
    against the options `against`): controls apart by more than 1e-6, or another evaluation count, or (constrained
    problems) another number of outer iterations."""
    (U, _, st), _ = reference_runs(O, cfg_kw, prob, k, ())
    (Ud, _, sd), _ = reference_runs(O, against or {}, prob, k, ())
    differs = (np.abs(U - Ud).max(1) > BITE_DU) | (st[:, 7] != sd[:, 7])
    if prob["base"]:
        differs |= st[:, 1] != sd[:, 1]
    return float(differs.mean())


def jitter_distances(plain, jittered, which=0):
    """max |difference| per agent of the controls (which = 0) or multipliers (which = 1), over the agents whose
    evaluation counts are equal -- what test_iterate_prefix_parity compares."""
    same = jittered[2][:, 7] == plain[2][:, 7]
    return same, np.abs(jittered[which] - plain[which]).max(1)[same]


# ----------------------------------------------------------------------------- the tables, regenerated
def _main():
    from oracle import oracle as O
    O.build()
    print("unconstrained prefixes: bite / stability (jitter seeds %s) per k" % (SEEDS,))
    for pname in UNC_SMALL + UNC_LARGE + ("pac20",):
        prob = problem(pname)
        print("  %s (model %d, N = %d, B = %d)" % (pname, prob["model"], prob["N"], prob["B"]))
        for e, kw in UNCONSTRAINED.items():
            print("    %-9s" % e + "  ".join("k=%d %.2f / %.2f" % (k, bite(O, kw, prob, k), stability(O, kw, prob, k))
                                             for k in UNC_KS), flush=True)
    print("ALM prefixes: outer iterations reached, most failed inner solves, bite / stability per k")
    for pname in ("lane", "squares"):
        prob = problem(pname)
        print("  %s (model %d, N = %d, B = %d)" % (pname, prob["model"], prob["N"], prob["B"]))
        for e in ["base"] + list(ALM):
            kw, used, against = ALM[e] if e in ALM else ({}, (), None)
            row = []
            for k in ALM_KS + (60,):
                st = reference_runs(O, kw, prob, k, ())[0][2]
                row.append("k=%d outer %d-%d fail<=%d %.2f / %.2f" % (k, st[:, 1].min(), st[:, 1].max(), st[:, 3].max(),
                                                                     alm_bite(O, e, prob, k) if e in ALM else 0.0,
                                                                     stability(O, kw, prob, k)))
            print("    %-14s" % e + "  ".join(row) + ("  (bite against %s)" % against if against else "")
                  + ("" if pname in used or e == "base" else "  (not used here)"), flush=True)
    print("the stalling agent: (status, outer, inner, failures, evaluations), seeds of %d with the same counts, "
          "largest max|dU| jittered vs plain" % len(STALL_SEEDS))
    prob = problem("stall")
    for e, (kw, _) in STALL.items():
        plain, jit = reference_runs(O, kw, prob, None, STALL_SEEDS)
        print("    %-17s %s  %d/%d  %.0e" % (e, tuple(int(v) for v in plain[2][0, COUNTS]),
                                             sum(bool(same_counts(j[2], plain[2])[0]) for j in jit), len(jit),
                                             max(np.abs(j[0] - plain[0]).max() for j in jit)), flush=True)


if __name__ == "__main__":
    _main()
