"""MPCController: drop-in for the reference's controller.MPCController (controller.py:10-69).

Same constructor, same `__call__(y_n, centerline) -> U` (flat NumPy [d0, delta0, d1, ...]),
same mutable attributes (`U`, `λ`, `tot_it`, `failures`, `N_horiz`, `u_dim`, `solver`,
`problem`, `model`).  Errors: like the reference, non-convergence raises nothing and only
increments `failures`.  Added for the batched use BASELINE.json asks for:
`solve(Y0, centerline) -> U[B, 2N]` and `step(Y0, centerline) -> u0[B, 2]` (= main.py:141).

The alpaqa ALM + structured PANOC arithmetic (controller.py:27-48, :57) runs in the
hand-written HIP kernels behind libmpc_hip.so.
"""
import numpy as np
import torch

from . import _lib
from .solver import BatchedMPC


def _tiled(vec, period, name):
    v = np.asarray(vec, dtype=np.float64).ravel()
    if v.size % period or not np.array_equal(v, np.tile(v[:period], v.size // period)):
        raise ValueError(f"{name} must repeat with period {period} over the horizon "
                         "(the kernels keep one bound per stage component)")
    return v[:period]


class MPCController:
    verbose = True  # the reference prints one status line per solve (controller.py:59-61)

    def __init__(self, model, problem, N_horiz):
        self.model = model
        self.problem = problem
        self.N_horiz = 12 if N_horiz is None else N_horiz
        N = int(self.N_horiz)
        self.u_dim = 2
        self.tot_it = 0
        self.failures = 0
        self.U = np.tile([1, 0], N)                       # controller.py:20
        nx = model.NX
        self.λ = np.zeros((nx * N,))                      # controller.py:21 (6 * N_horiz for nx = 6)

        S = int(problem.centerline_size)
        veh = np.asarray(problem.param[nx + 2 * S:], dtype=np.float64)
        lb = _tiled(problem.C.lowerbound, 2, "problem.C.lowerbound")   # main.py:55
        ub = _tiled(problem.C.upperbound, 2, "problem.C.upperbound")   # main.py:56
        Dlb = _tiled(problem.D.lowerbound, nx, "problem.D.lowerbound")
        Dub = _tiled(problem.D.upperbound, nx, "problem.D.upperbound")
        constrained = bool(np.any(np.isfinite(Dlb)) or np.any(np.isfinite(Dub)))
        # problem.keep_out_discs (not in the reference): the general constraints are keep-out discs per agent and stage
        # (CONSTR_DISCS), supplied to solve() / step() as discs= ; problem.D is then not read
        discs = bool(getattr(problem, "keep_out_discs", False))
        pad = [0.0] * (6 - nx)
        # controller.py:27-48: ProjGradNorm2, max_iter 1000, heuristic 15, memory N_horiz,
        # eps 1e-6, delta 1e-4, Sigma_0 1e5, outer max_iter 1000 (mpc_default_config holds them)
        self.cfg = _lib.default_config(
            model.MODEL_ID, N, S=S, Ts=float(model.Ts), v_ref=float(problem.v_ref), veh=list(veh),
            u_lb=list(lb), u_ub=list(ub), lbfgs_memory=N,
            constr_mode=_lib.CONSTR_DISCS if discs else _lib.CONSTR_STATE_SQ if constrained else _lib.CONSTR_NONE,
            D_lb=list(Dlb) + [-np.inf] * len(pad), D_ub=list(Dub) + [np.inf] * len(pad),
            wrap_mode=int(getattr(problem, "wrap_mode", _lib.WRAP_FLOOR)),
            max_total_inner=int(getattr(problem, "max_total_inner", 5000)))
        self.solver = BatchedMPC(self.cfg)
        self.device = self.solver.device
        self._veh0 = veh.copy()      # the vehicle part of problem.param the handle was created from
        self._nx, self._S = nx, S
        self._constrained = constrained or discs
        self.last_stats = None

    # ------------------------------------------------------------------ reference entry point
    def __call__(self, y_n, centerline):
        y_n = np.array(y_n, dtype=np.float64).ravel()
        centerline = np.asarray(centerline, dtype=np.float64).ravel()
        # controller.py:54: the current state and centerline are parameters of the problem
        self.problem.param[:(y_n.shape[0] + centerline.shape[0])] = np.concatenate((y_n, centerline))
        dev = self.device
        x0 = torch.as_tensor(y_n[None, :], device=dev)
        cl = torch.as_tensor(centerline[None, :], device=dev)
        U0 = torch.as_tensor(np.asarray(self.U, dtype=np.float64)[None, :], device=dev)
        lam0 = torch.as_tensor(np.asarray(self.λ, dtype=np.float64)[None, :], device=dev) \
            if self._constrained else None
        # main.py:119: the vehicle parameters are run-time data of the problem.  A caller who has rewritten them in
        # problem.param since construction is served through a one-row parameter table holding the new values;
        # unchanged parameters take the handle's own path.
        veh = np.asarray(self.problem.param[self._nx + 2 * self._S:], dtype=np.float64)
        changed = veh.shape != self._veh0.shape or not np.array_equal(veh, self._veh0)
        if changed:
            row = _lib.param_rows(self.cfg, 1, veh=veh)
            self.solver.set_agent_params(torch.as_tensor(row, device=dev).contiguous(),
                                         torch.zeros(1, dtype=torch.int32, device=dev))
        try:
            # controller.py:57: warm start from the previous solution and multipliers
            U, lam, stats = self.solver.solve(x0.contiguous(), cl.contiguous(), U0.contiguous(), lam0)
        finally:
            if changed:
                self.solver.clear_agent_params()
        st = stats.cpu().numpy()[0]
        self.U = U.cpu().numpy()[0]
        if lam is not None:
            self.λ = lam.cpu().numpy()[0]
        self.last_stats = st
        if self.verbose:  # controller.py:59-61
            print(_status_name(int(st[0])), int(st[1]), int(st[2]), int(st[3]))
        self.tot_it += int(st[2])                              # controller.py:63
        self.failures += int(st[0]) != _lib.ST_CONVERGED       # controller.py:64
        return self.U                                          # controller.py:69

    # ------------------------------------------------------------------ batched entry points
    def solve(self, Y0, centerline, U0=None, lam0=None, cl_index=None, params=None, param_index=None,
              bounds=None, bound_index=None, constraints=None, constraint_index=None, roads=None, road_index=None,
              fields=None, field_index=None, discs=None, disc_index=None, rates=None, rate_index=None):
        """Batched solve: Y0 [B, nx], centerline [2S] or [C, 2S] (+ cl_index[B]) -> (U [B, 2N], stats).
        params [P, 31] (rows as _lib.param_rows makes them) + param_index [B] (None: agent b uses row b % P): this
        solve runs agent b on its own vehicle and cost parameters (BatchedMPC.set_agent_params).
        bounds [P', 4] (rows as _lib.bound_rows makes them) + bound_index [B] (None: agent b uses row b % P'): this solve
        projects agent b's inputs onto its own box (BatchedMPC.set_agent_bounds).
        constraints [P", 19] (rows as _lib.constraint_rows makes them) + constraint_index [B] (None: agent b uses row
        b % P"): this solve holds agent b to its own constraint data (BatchedMPC.set_agent_constraints).
        discs [P°, 6N] (rows as _lib.disc_rows makes them) + disc_index [B] (None: agent b uses row b % P°): this solve
        keeps agent b out of the discs of its own row, stage by stage (BatchedMPC.set_agent_discs; a controller whose
        problem has keep_out_discs set needs them in every solve).
        rates [P*, 4] (rows as _lib.rate_rows makes them) + rate_index [B] (None: agent b uses row b % P*): this solve
        penalises agent b's input moves with the weights, and from the last applied input, of its own row
        (BatchedMPC.set_agent_rates; not together with constraints=).
        fields [P', N, NFIELD, NFSRC] or [P', 16 N] (as _lib.field_rows makes them) + field_index [B] (None: agent b uses
        row b % P'): this solve adds the risk field of its own row to agent b's cost, stage by stage
        (BatchedMPC.set_agent_fields; not together with constraints= or discs=).
        roads [P', N, NROAD] or [P', 8 N] (as _lib.road_rows makes them) + road_index [B] (None: agent b uses row b % P'):
        this solve adds the lane target, the soft road edges and the speed target of its own row to agent b's cost, stage
        by stage (BatchedMPC.set_agent_roads; beside discs= too, not together with constraints=).
        Pass the tables by keyword: roads=, road_index=, fields= and field_index= stand in front of discs=, so the
        positional slots behind constraint_index have moved with every table added there."""
        dev = self.device
        Y0 = torch.as_tensor(Y0, dtype=torch.float64, device=dev).contiguous()
        B = Y0.shape[0]
        cl = torch.as_tensor(centerline, dtype=torch.float64, device=dev).contiguous()
        if U0 is None:
            U0 = torch.tensor([1.0, 0.0], dtype=torch.float64, device=dev).repeat(B, int(self.N_horiz))
        else:
            U0 = torch.as_tensor(U0, dtype=torch.float64, device=dev).contiguous()
        if cl_index is not None:
            cl_index = torch.as_tensor(cl_index, dtype=torch.int32, device=dev).contiguous()
        if lam0 is not None:
            lam0 = torch.as_tensor(lam0, dtype=torch.float64, device=dev).contiguous()
        tables = []                                       # (kind, table, index) of the tables this call binds
        for kind, table, index, name in (("params", params, param_index, "param_index"),
                                         ("bounds", bounds, bound_index, "bound_index"),
                                         ("constraints", constraints, constraint_index, "constraint_index"),
                                         ("discs", discs, disc_index, "disc_index"),
                                         ("rates", rates, rate_index, "rate_index"),
                                         ("fields", fields, field_index, "field_index"),
                                         ("roads", roads, road_index, "road_index")):
            if table is None:
                if index is not None:
                    raise ValueError(f"{name} needs {kind}")
                continue
            table = torch.as_tensor(table, dtype=torch.float64, device=dev).contiguous()
            if (kind == "fields" and table.dim() == 4) or (kind == "roads" and table.dim() == 3):
                table = table.reshape(table.shape[0], -1)
            if index is None:
                index = torch.arange(B, device=dev) % table.shape[0]
            tables.append((kind, table, torch.as_tensor(index, device=dev).to(torch.int32).contiguous()))
        try:
            for kind, table, index in tables:
                getattr(self.solver, "set_agent_" + kind)(table, index)
            U, lam, stats = self.solver.solve(Y0, cl, U0, lam0 if self._constrained else None, cl_index)
        finally:
            for kind, _, _ in tables:
                getattr(self.solver, "clear_agent_" + kind)()
        self.last_stats = stats
        self.tot_it += int(stats[:, 2].sum().item())
        self.failures += int((stats[:, 0] != _lib.ST_CONVERGED).sum().item())
        return U, stats

    def step(self, Y0, centerline, U0=None, lam0=None, cl_index=None, params=None, param_index=None,
             bounds=None, bound_index=None, constraints=None, constraint_index=None, roads=None, road_index=None,
             fields=None, field_index=None, discs=None, disc_index=None, rates=None, rate_index=None):
        """First control of every agent, u0 [B, 2] (main.py:141 input_to_matrix(U)[:, 0])."""
        U, _ = self.solve(Y0, centerline, U0, lam0, cl_index, params, param_index, bounds, bound_index,
                          constraints, constraint_index, roads, road_index, fields, field_index, discs, disc_index, rates,
                          rate_index)
        return U[:, :2].contiguous()


_STATUS = {0: "SolverStatus.Unknown", 1: "SolverStatus.Converged", 2: "SolverStatus.MaxTime",
           3: "SolverStatus.MaxIter", 4: "SolverStatus.NotFinite", 5: "SolverStatus.NoProgress",
           6: "SolverStatus.Interrupted"}


def _status_name(code):
    return _STATUS.get(code, f"SolverStatus({code})")
