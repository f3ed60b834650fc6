"""BatchedMPC: torch-tensor front end of the C-ABI (include/mpc_hip.h).

Holds no arithmetic of its own: it checks shapes/dtypes/devices on the host (a
wrong shape handed to a hand-written kernel is a GPU fault) and forwards raw
device pointers plus the current HIP stream.
"""
import collections
import ctypes as C

import torch

from . import _lib


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# what BatchedMPC.closed_loop_event returns: the final states x [B, nx], the plans U as last solved, the multipliers,
# held [B] (stages of the plan already applied), traj_x [B, T, nx], traj_u [B, T, 2], solved [B, T] uint8,
# solve_count [B], failures [B] and stats [B, 8] of each agent's most recent solve
EventLoopResult = collections.namedtuple(
    "EventLoopResult", "x U lam held traj_x traj_u solved solve_count failures stats")

# what BatchedMPC.closed_loop_track returns: the fields of EventLoopResult, then cl_index [B] int32 (each agent's row of
# the window table on return: pass it to the next call) and traj_row [B, T] int32 (the row in force at every step)
TrackLoopResult = collections.namedtuple(
    "TrackLoopResult", EventLoopResult._fields + ("cl_index", "traj_row"))

# what BatchedMPC.closed_loop_traffic returns: what closed_loop returns -- x, U, lam, traj_x [B, T, nx], traj_u [B, T, 2],
# failures [B], stats [B, 8] of the last solve --, then traj_opp [B, T, NDISC] int32 (the opponents every agent avoided at
# every step, -1: none), traj_clear [B, T] (the clearance d^2 - r^2 to the nearest agent of the scene after every step)
# and the disc table [B, 3 NDISC N] as the last step left it (bound to the engine)
TrafficLoopResult = collections.namedtuple(
    "TrafficLoopResult", "x U lam traj_x traj_u failures stats traj_opp traj_clear table")

# what BatchedMPC.closed_loop_obstacles returns: what closed_loop returns -- x, U, lam, traj_x [B, T, nx], traj_u [B, T, 2],
# failures [B], stats [B, 8] of the last solve --, then traj_sel [B, T, NDISC] int32 (the obstacles of its scene every agent
# avoided at every step, -1: none), traj_clear [B, T] (the clearance to the nearest present obstacle after every step), the
# disc or field table as the last step left it (bound to the engine) and cl_index [B] int32 (with a track: every agent's
# row of the window table on return; else what was passed)
ObstacleLoopResult = collections.namedtuple(
    "ObstacleLoopResult", "x U lam traj_x traj_u failures stats traj_sel traj_clear table cl_index")

# what BatchedMPC.closed_loop_obstacles_event returns: the fields of ObstacleLoopResult (U: the plans as last solved, not
# shifted by the stages applied since), then solved [B, T] uint8, solve_count [B], held [B] int32 (stages of the plan
# already applied), sel_plan [B, NDISC] int32 (the obstacles every agent's plan was solved against) and traj_why [B, T]
# uint8 (bit 0: the car trigger -- deviation, hold limit, no plan --, bit 1: clearance, bit 2: a new obstacle)
ObstacleEventLoopResult = collections.namedtuple(
    "ObstacleEventLoopResult", ObstacleLoopResult._fields + ("solved", "solve_count", "held", "sel_plan", "traj_why"))

# what BatchedMPC.closed_loop_traffic_event returns: the fields of TrafficLoopResult (U: the plans as last solved, not
# shifted by the stages applied since), then solved [B, T] uint8, solve_count [B], held [B] int32 (stages of the plan
# already applied), opp_plan [B, NDISC] int32 (the agents every agent's plan was solved against, global indices) and
# traj_why [B, T] uint8 (bit 0: the car trigger, bit 1: clearance to the others' plans, bit 2: a new opponent)
TrafficEventLoopResult = collections.namedtuple(
    "TrafficEventLoopResult", TrafficLoopResult._fields + ("solved", "solve_count", "held", "opp_plan", "traj_why"))


class Track:
    """A table of track windows (BatchedMPC.track_windows): `win` [K * R, 2S], the window tensor -- an ordinary
    centerline table, usable wherever one is --, `track` [K, 2L] it was gathered from and the geometry K, L, S, stride,
    lead, closed, R (include/mpc_hip.h: mpc_track).  Holds both tensors alive."""

    def __init__(self, geom, S, track, win):
        self._c = geom
        self.K, self.L, self.stride, self.lead = int(geom.K), int(geom.L), int(geom.stride), int(geom.lead)
        self.closed, self.R, self.S = bool(geom.closed), int(geom.R), int(S)
        self.track, self.win = track, win

    @property
    def rows(self):
        return self.K * self.R

    def __repr__(self):
        return (f"Track(K={self.K}, L={self.L}, S={self.S}, stride={self.stride}, lead={self.lead}, "
                f"closed={self.closed}, R={self.R})")


# the per-agent tables of an engine, by kind: doubles per row (and per stage of the engine's horizon on top), the
# library's setter, whether the setter takes a plant index
_AgentTable = collections.namedtuple("_AgentTable", "width width_per_N setter plant")
_AGENT_TABLES = {"params": _AgentTable(_lib.NPARAM, 0, "mpc_set_agent_params", True),
                 "bounds": _AgentTable(_lib.NBOUND, 0, "mpc_set_agent_bounds", False),
                 "constraints": _AgentTable(_lib.NCONSTR, 0, "mpc_set_agent_constraints", False),
                 "discs": _AgentTable(0, 3 * _lib.NDISC, "mpc_set_agent_discs", False),
                 "rates": _AgentTable(_lib.NRATE, 0, "mpc_set_agent_rates", False),
                 "fields": _AgentTable(0, _lib.NFIELD * _lib.NFSRC, "mpc_set_agent_fields", False),
                 "roads": _AgentTable(0, _lib.NROAD, "mpc_set_agent_roads", False)}


class BatchedMPC:
    """One handle = one GPU.  All tensors are float64, contiguous, on `device`."""

    def __init__(self, cfg, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedMPC needs a HIP device (no CPU fallback exists)")
        self.lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None \
            else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("device must be a HIP (cuda) device")
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        self.cfg = cfg
        self.N = int(cfg.N)
        self.S = int(cfg.S)
        self.nx = self.lib.mpc_nx(C.byref(cfg))
        self.n = 2 * self.N
        self.m = self.lib.mpc_m(C.byref(cfg))
        self.M = int(cfg.lbfgs_memory)
        h = C.c_void_p()
        _lib.check(self.lib.mpc_create(C.byref(cfg), idx, C.byref(h)))
        self._h = h
        self._pending = False       # an asynchronous solve is in flight: the worker thread owns the handle
        self._cl_key, self._cl_keep = None, None   # the centerline table the search tables were last built for
        self._keep = {}             # kind -> (table, index[, plant_index]) of set_agent_<kind>, alive while bound
        import os
        # nearest-point search of K1b as the library chose it at mpc_create: 2 grid of index ranges (default), 0 the
        # full scan (MPC_NEAREST_SCAN) -- which needs no tables
        self._nearest_blocks = 0 if "MPC_NEAREST_SCAN" in os.environ else 2

    def close(self):
        if getattr(self, "_h", None):
            self.lib.mpc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _free(self):
        """Refuse a call on an engine whose asynchronous solve has not been collected -- before anything
        touches the handle (the library refuses too; its tables and workspace belong to the worker)."""
        if self._pending:
            raise _lib.MpcError("a solve of this engine is in flight: call the function solve_async returned first")

    def _chk(self, t, shape, name, dtype=torch.float64):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a torch.Tensor")
        if t.dtype != dtype:
            raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
        if t.device != self.device:
            raise ValueError(f"{name}: expected device {self.device}, got {t.device}")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: must be contiguous")
        return t

    def _centerline(self, cl, cl_index, B):
        self._free()
        if cl.dim() == 1:
            cl = cl.unsqueeze(0)
        if cl.dim() != 2 or cl.shape[1] != 2 * self.S:
            raise ValueError(f"centerline: expected [C, {2 * self.S}] (flat x.. then y..), "
                             f"got {tuple(cl.shape)}")
        self._chk(cl, cl.shape, "centerline")
        if cl_index is not None:
            self._chk(cl_index, (B,), "cl_index", torch.int32)
            if B and (int(cl_index.min()) < 0 or int(cl_index.max()) >= cl.shape[0]):
                raise ValueError("cl_index out of range")
        if self._nearest_blocks:
            # f-2: the tables of the pruned nearest-point searches for this centerline table (three small
            # kernels: ~30 us for one row, but 65 536 cells x 2 (S - 1) points and 256 KB of cells PER ROW for a
            # table of many rows).
            # A ONE-ROW table (the shared centerline of main.py) is rebuilt on every call: the caller may have
            # refreshed it in place by any route -- `cl.data.copy_()`, DLPack, a raw kernel -- and no host-side
            # key sees all of them; 30 us on a solve of milliseconds.
            # A table of SEVERAL rows is rebuilt only when it is another table or its contents have changed: the
            # key holds the address, the shape, torch's in-place write counter, the stream (the tables are built by
            # kernels on the caller's current stream, and a call on another stream must not read them before those
            # kernels have run) AND a checksum of the table's bits computed on the device at every call (one
            # reduction over C x 2S words, ~20 us, against ~1 ms of table building per 64 rows) -- a write behind
            # torch's back (`.data`, DLPack, a raw kernel) changes the checksum.  The engine keeps the tensor
            # alive meanwhile, so its address cannot be handed to another table.
            if cl.shape[0] == 1:
                self._cl_key, self._cl_keep = None, None
                _lib.check(self.lib.mpc_centerline_blocks(self._h, _ptr(cl), 1, self._stream()))
            else:
                key = (cl.data_ptr(), tuple(cl.shape), cl._version, self._nearest_blocks,
                       torch.cuda.current_stream(self.device).cuda_stream, int(cl.view(torch.int64).sum().item()))
                if key != self._cl_key:
                    self._cl_key, self._cl_keep = None, None
                    _lib.check(self.lib.mpc_centerline_blocks(self._h, _ptr(cl), int(cl.shape[0]), self._stream()))
                    self._cl_key, self._cl_keep = key, cl
        return cl

    # ------------------------------------------------------------------ per-agent tables
    def _bind_agent_table(self, kind, table, *indices):
        """set_agent_<kind>: the shape, dtype, device and range checks, the library's setter, and the tensors kept alive.
        indices: `index`, and `plant_index` (or None) for the kind that has one."""
        d, width = _AGENT_TABLES[kind], self._table_width(kind)
        self._free()
        if not isinstance(table, torch.Tensor) or table.dim() != 2 or table.shape[1] != width or table.shape[0] < 1:
            raise ValueError(f"table: expected a tensor [P >= 1, {width}]")
        self._chk(table, table.shape, "table")
        index = indices[0]
        if not isinstance(index, torch.Tensor) or index.dim() != 1 or index.shape[0] < 1:
            raise ValueError("index: expected a tensor [B >= 1]")
        B, P = int(index.shape[0]), int(table.shape[0])
        for t, name in zip(indices, ("index", "plant_index")):
            if t is None:
                continue
            self._chk(t, (B,), name, torch.int32)
            if int(t.min()) < 0 or int(t.max()) >= P:
                raise ValueError(f"{name} out of range")
        _lib.check(getattr(self.lib, d.setter)(self._h, _ptr(table), P, *map(_ptr, indices), B))
        self._keep[kind] = (table, *indices)

    def _clear_agent_table(self, kind):
        d = _AGENT_TABLES[kind]
        self._free()
        _lib.check(getattr(self.lib, d.setter)(self._h, None, 0, *([None] * (2 if d.plant else 1)), 0))
        self._keep.pop(kind, None)

    def set_agent_params(self, table, index, plant_index=None):
        """Binds a per-agent parameter table (mpc_set_agent_params): table [P, 31] float64 (rows as
        _lib.param_rows makes them), index [B] int32 = the row of agent b, plant_index [B] int32 = the row the PLANT
        of closed_loop advances with (None: the same).  Bound, every model-dependent call (rhs, rollout, stage_cost,
        eval_cost_grad, solve, solve_async, closed_loop) uses agent b's row and serves batches of exactly B agents.
        The tensors stay the caller's: the library reads them at every call, so rows may be rewritten in place
        between calls; the engine keeps them alive until clear_agent_params()."""
        self._bind_agent_table("params", table, index, plant_index)

    def clear_agent_params(self):
        """Unbinds the parameter table: the engine is what it was before set_agent_params."""
        self._clear_agent_table("params")

    @property
    def agent_params_bound(self):
        return "params" in self._keep

    def set_agent_bounds(self, table, index):
        """Binds a per-agent table of input boxes (mpc_set_agent_bounds): table [P, 4] float64 (rows
        [u_lb[0], u_lb[1], u_ub[0], u_ub[1]], as _lib.bound_rows makes them), index [B] int32 = the row of agent b.
        Bound, every call that projects onto the box (prox_step, solve, solve_async, solve_active, closed_loop,
        closed_loop_event) uses agent b's row and serves batches of exactly B agents.  Independent of the parameter
        table (either, both or neither; together they are for the same B).  The tensors stay the caller's: the
        library reads them at every call, so rows may be rewritten in place between calls; the engine keeps them
        alive until clear_agent_bounds()."""
        self._bind_agent_table("bounds", table, index)

    def clear_agent_bounds(self):
        """Unbinds the bounds table: the engine is what it was before set_agent_bounds."""
        self._clear_agent_table("bounds")

    @property
    def agent_bounds_bound(self):
        return "bounds" in self._keep

    def set_agent_constraints(self, table, index):
        """Binds a per-agent table of constraint data (mpc_set_agent_constraints): table [P, 19] float64 (rows
        [g_off[6], D_lb[6], D_ub[6], lane_halfwidth], as _lib.constraint_rows makes them; only the fields of the engine's
        constr_mode are read), index [B] int32 = the row of agent b.  Bound, every call that reads constraint data
        (eval_cost_grad, solve, solve_async, solve_active, closed_loop, closed_loop_event) uses agent b's row and serves
        batches of exactly B agents.  Independent of the parameter and bounds tables (any subset; together they are for
        the same B).  The tensors stay the caller's: the library reads them at every call, so rows may be rewritten in
        place between calls; the engine keeps them alive until clear_agent_constraints()."""
        self._bind_agent_table("constraints", table, index)

    def clear_agent_constraints(self):
        """Unbinds the constraint table: the engine is what it was before set_agent_constraints."""
        self._clear_agent_table("constraints")

    @property
    def agent_constraints_bound(self):
        return "constraints" in self._keep

    def set_agent_discs(self, table, index):
        """Binds a per-agent table of keep-out discs (mpc_set_agent_discs; an engine of CONSTR_DISCS alone): table
        [P, 3 * NDISC * N] float64 (rows [N][NDISC][3] = (cx, cy, r), as _lib.disc_rows makes them; r = 0: no obstacle),
        index [B] int32 = the row of agent b.  An engine of CONSTR_DISCS needs it bound in every call that evaluates
        constraints (eval_cost_grad, solve, solve_async, solve_active, the closed loops); they use agent b's row, stage k of
        the horizon reading entry k, and serve batches of exactly B agents.  Independent of the parameter and bounds
        tables (together they are for the same B).  The tensors stay the caller's: the library reads them at every call,
        so rows may be rewritten in place between calls (moving obstacles in a host loop of solves); the engine keeps
        them alive until clear_agent_discs()."""
        self._bind_agent_table("discs", table, index)

    def clear_agent_discs(self):
        """Unbinds the disc table (an engine of CONSTR_DISCS then refuses to evaluate until one is bound again)."""
        self._clear_agent_table("discs")

    @property
    def agent_discs_bound(self):
        return "discs" in self._keep

    def set_agent_rates(self, table, index):
        """Binds a per-agent table of move penalties (mpc_set_agent_rates): table [P, 4] float64 (rows
        [w_d, w_delta, d_prev, delta_prev], as _lib.rate_rows makes them), index [B] int32 = the row of agent b.  Bound,
        every call that evaluates the horizon's cost (eval_cost_grad(_wave), solve, solve_async, solve_active, the closed
        loops) adds w_d (d_k - d_{k-1})^2 + w_delta (delta_k - delta_{k-1})^2 to stage k of agent b, u_{-1} being the
        row's (d_prev, delta_prev), and serves batches of exactly B agents.  Beside the parameter, bounds and disc tables
        (together they are for the same B); not beside a constraint table.  The tensors stay the caller's: the library
        reads them at every call, so rows may be rewritten in place between calls (a host loop writes the input it
        applies into columns 2 and 3; the closed loops do that themselves and need P == B with index = arange(B)); the
        engine keeps them alive until clear_agent_rates()."""
        self._bind_agent_table("rates", table, index)

    def clear_agent_rates(self):
        """Unbinds the rate table: the engine is what it was before set_agent_rates."""
        self._clear_agent_table("rates")

    @property
    def agent_rates_bound(self):
        return "rates" in self._keep

    def _check_rate_rows(self, B):
        """What the closed loops ask of a bound rate table: they write the applied input into agent b's own row."""
        if "rates" not in self._keep:
            return
        table, index = self._keep["rates"]
        if int(table.shape[0]) != B or int(index.shape[0]) != B:
            raise ValueError(f"the bound rate table has {int(table.shape[0])} rows for {int(index.shape[0])} agents: a closed loop "
                             f"needs one row per agent (P == B = {B}, index = arange(B))")
        if not torch.equal(index, torch.arange(B, dtype=torch.int32, device=index.device)):
            raise ValueError("the bound rate table's index is not arange(B): a closed loop writes the applied input into row b of agent b")

    # ------------------------------------------------------------------ what the closed loops share
    def _table_width(self, kind):
        return _AGENT_TABLES[kind].width + _AGENT_TABLES[kind].width_per_N * self.N

    def _multipliers(self, B, lam, inplace=False):
        """lam [B, m] of a call that writes it: zeros when None, else the caller's (a copy unless inplace), checked; None on
        an engine without constraints"""
        if not self.m:
            return None
        lam = torch.zeros(B, self.m, dtype=torch.float64, device=self.device) if lam is None else (lam if inplace else lam.clone())
        return self._chk(lam, (B, self.m), "lam")

    def _loop_entry(self, x, U):
        """B of a closed loop on x [B, nx] and U [B, 2N], a bound rate table being one a loop can write"""
        B = x.shape[0]
        self._chk(x, (B, self.nx), "x"); self._chk(U, (B, self.n), "U")
        self._check_rate_rows(B)
        return B

    def _loop_state(self, B, T, x, U, lam, stats=True):
        """(x, U, lam, traj_x, traj_u, failures, stats) of a closed loop: copies of what the caller passed and what the
        library fills (stats=False: None in place of a fresh stats, for the loops that continue the caller's)"""
        x, U = x.clone(), U.clone()
        lam = self._multipliers(B, lam)
        tx, tu = self._empty(B, T, self.nx), self._empty(B, T, 2)
        fails = torch.zeros(B, dtype=torch.int32, device=self.device)
        return x, U, lam, tx, tu, fails, self._empty(B, _lib.NSTATS) if stats else None

    def _event_loop_state(self, B, T, x, U, lam, held, disturbance, stats):
        """the fields of an EventLoopResult, in its order: _loop_state with the caller's held (None: -1, no plan yet) and
        stats (None: zeros) copied, solved and solve_count; disturbance [B, T, nx] is checked"""
        held = torch.full((B,), -1, dtype=torch.int32, device=self.device) if held is None else held.clone()
        self._chk(held, (B,), "held", torch.int32)
        x, U, lam, tx, tu, fails, _ = self._loop_state(B, T, x, U, lam, stats=False)
        if disturbance is not None:
            self._chk(disturbance, (B, T, self.nx), "disturbance")
        stats = torch.zeros(B, _lib.NSTATS, dtype=torch.float64, device=self.device) if stats is None else stats.clone()
        self._chk(stats, (B, _lib.NSTATS), "stats")
        solved = torch.zeros(B, T, dtype=torch.uint8, device=self.device)
        count = torch.zeros(B, dtype=torch.int32, device=self.device)
        return x, U, lam, held, tx, tu, solved, count, fails, stats

    def _loop_table(self, kind, B, table, identity_index=False):
        """The table of `kind` ("discs" or "fields") that a loop rewrites in place: None -- zeros, bound with arange(B) and
        left bound; else the caller's, checked.  identity_index: a bound table whose index is not arange(B) is refused --
        closed_loop_obstacles alone asks for that; the traffic loops leave the index to the caller, as the library does
        (an asymmetry kept as it was found)."""
        if table is None:
            table = torch.zeros(B, self._table_width(kind), dtype=torch.float64, device=self.device)
            self._bind_agent_table(kind, table, torch.arange(B, dtype=torch.int32, device=self.device))
            return table
        self._chk(table, (B, self._table_width(kind)), "table")
        if identity_index and kind in self._keep and self._keep[kind][0] is table and \
                not torch.equal(self._keep[kind][1], torch.arange(B, dtype=torch.int32, device=self.device)):
            raise ValueError(f"the bound {kind[:-1]} table's index is not arange(B): the loop writes row b for agent b")
        return table

    def _check_scene(self, B, G):
        """scenes are blocks of G consecutive agents"""
        if not 1 <= G <= _lib.SCENE_MAX:
            raise ValueError(f"G: a scene holds 1 .. {_lib.SCENE_MAX} agents")
        if B % G:
            raise ValueError(f"the batch of {B} agents is not a whole number of scenes of {G} (pad the scenes)")

    def _plans(self, X):
        """(X, B, Nst) of a selection on plans X [B, Nst >= 1, nx]; [B, nx] is one stage, the states as they are now"""
        self._free()
        if isinstance(X, torch.Tensor) and X.dim() == 2:
            X = X.unsqueeze(1)
        if not isinstance(X, torch.Tensor) or X.dim() != 3 or X.shape[1] < 1:
            raise ValueError(f"X: expected [B, Nst >= 1, {self.nx}]")
        B, Nst = int(X.shape[0]), int(X.shape[1])
        return self._chk(X, (B, Nst, self.nx), "X"), B, Nst

    def _rows_from_plans(self, fn, kind, X, opp, per, per_name, out):
        """discs_from_plans / fields_from_plans: X [B, N, nx], opp [B, NDISC] int32, `per` [B, ...] (agent b as an obstacle)
        and the table of `kind`, `out` or a new one"""
        self._free()
        if not isinstance(X, torch.Tensor) or X.dim() != 3:
            raise ValueError(f"X: expected [B, {self.N}, {self.nx}]")
        B = X.shape[0]
        self._chk(X, (B, self.N, self.nx), "X")
        assert _lib.NDISC == _lib.NFIELD        # one opp [B, 2] serves the discs and the fields, as in the library
        self._chk(opp, (B, _lib.NDISC), "opp", torch.int32)
        self._chk(per, (B,) if kind == "discs" else (B, 4), per_name)
        width = self._table_width(kind)
        table = self._empty(B, width) if out is None else self._chk(out, (B, width), "out")
        _lib.check(fn(self._h, B, _ptr(X), _ptr(opp), _ptr(per), _ptr(table), self._stream()))
        return table

    def set_agent_fields(self, table, index):
        """Binds a per-agent table of risk fields (mpc_set_agent_fields; not on an engine of CONSTR_DISCS): table
        [P, NFIELD * NFSRC * N] float64 (rows [N][NFIELD][NFSRC], sources [cx, cy, c, s, A, kx, ky, alpha], as
        _lib.field_rows(...).reshape(P, -1) makes them; A = 0: no source), index [B] int32 = the row of agent b.  Bound,
        every call that evaluates the horizon's cost (eval_cost_grad(_wave), solve, solve_async, solve_active, the closed
        loops) adds the skewed Gaussians of agent b's row to its stage costs, stage k reading entry k, and serves batches
        of exactly B agents.  A cost, not a constraint: it works beside the engine's own constraint data (a lane band),
        the parameter, bounds and rate tables (together they are for the same B); not beside a constraint table.  The
        tensors stay the caller's: the library reads them at every call, so rows may be rewritten in place between
        calls; the engine keeps them alive until clear_agent_fields()."""
        self._bind_agent_table("fields", table, index)

    def clear_agent_fields(self):
        """Unbinds the field table: the engine is what it was before set_agent_fields."""
        self._clear_agent_table("fields")

    @property
    def agent_fields_bound(self):
        return "fields" in self._keep

    def set_agent_roads(self, table, index):
        """Binds a per-agent table of road data (mpc_set_agent_roads; an engine of any constr_mode, CONSTR_DISCS included):
        table [P, NROAD * N] float64 (rows [N][NROAD], stage entries [off, w_off, lo, w_lo, hi, w_hi, v_tgt, w_v], as
        _lib.road_rows(...).reshape(P, -1) makes them; a weight of 0: that part is off), index [B] int32 = the row of
        agent b.  Bound, every call that evaluates the horizon's cost (eval_cost_grad(_wave), solve, solve_async,
        solve_active, the closed loops) adds the lane target, the soft road edges and the speed target of agent b's row to
        its stage costs, stage k reading entry k, and serves batches of exactly B agents.  The lateral offset e is the
        lane band's, positive to the right of the direction of travel.  A cost, not a constraint: it works beside the
        engine's own constraint data, the disc table of an engine of CONSTR_DISCS, and the parameter, bounds, rate and
        field tables (together they are for the same B); not beside a constraint table.  The tensors stay the caller's:
        the library reads them at every call, so rows may be rewritten in place between calls (roads_from_script does);
        the engine keeps them alive until clear_agent_roads()."""
        self._bind_agent_table("roads", table, index)

    def clear_agent_roads(self):
        """Unbinds the road table: the engine is what it was before set_agent_roads."""
        self._clear_agent_table("roads")

    @property
    def agent_roads_bound(self):
        return "roads" in self._keep

    def roads_from_script(self, script, index, ti, wrap=False, out=None):
        """mpc_roads_from_script: the road table [B, NROAD * N] whose row b is the window of N samples from sample `ti`
        of script row index[b] -- script [Ps, Lt, NROAD] float64 (one sample per Ts, entries as _lib.road_rows makes
        them), index [B] int32 in [0, Ps).  Stage k gets sample min(ti + k, Lt - 1), or (ti + k) % Lt with wrap.  A copy
        on the current stream; `out`: a table to write in place (the bound one, say), else a new one.  The samples are
        not checked: the script is the caller's to keep valid."""
        self._free()
        if not isinstance(script, torch.Tensor) or script.dim() != 3 or script.shape[0] < 1 or script.shape[1] < 1:
            raise ValueError(f"script: expected [Ps >= 1, Lt >= 1, {_lib.NROAD}]")
        Ps, Lt = int(script.shape[0]), int(script.shape[1])
        self._chk(script, (Ps, Lt, _lib.NROAD), "script")
        if not isinstance(index, torch.Tensor) or index.dim() != 1:
            raise ValueError("index: expected a tensor [B]")
        B = int(index.shape[0])
        self._chk(index, (B,), "index", torch.int32)
        if B and (int(index.min()) < 0 or int(index.max()) >= Ps):
            raise ValueError("index out of range")
        ti = int(ti)
        if ti < 0:
            raise ValueError("ti must be >= 0")
        width = _lib.NROAD * self.N
        table = self._empty(B, width) if out is None else self._chk(out, (B, width), "out")
        _lib.check(self.lib.mpc_roads_from_script(self._h, B, Lt, int(bool(wrap)), ti, _ptr(script), _ptr(index), _ptr(table),
                                                  self._stream()))
        return table

    def fields_from_plans(self, X, opp, shape, out=None):
        """mpc_fields_from_plans: the field table [B, NFIELD * NFSRC * N] in which agent b's sources are the plans of its
        opponents -- X [B, N, nx] as rollout() returns it for the agents' current plans, opp [B, NFIELD] int32 (the
        opponents of agent b, as opponents_from_plans returns them; < 0 or >= B: none, eight zeros), shape [B, 4] =
        [A, kx, ky, gain] of agent b as an obstacle: the source sits at the opponent's planned position in the frame of
        its planned heading, skewed by gain * (own speed - its speed).  A gather on the current stream; `out`: a table to
        write in place (one that is bound, say), else a new one."""
        return self._rows_from_plans(self.lib.mpc_fields_from_plans, "fields", X, opp, shape, "shape", out)

    def discs_from_plans(self, X, opp, radius, out=None):
        """mpc_discs_from_plans: the disc table [B, 3 * NDISC * N] in which agent b's discs are the plans of its
        opponents -- X [B, N, nx] as rollout() returns it for the agents' current plans, opp [B, NDISC] int32 (the
        opponents of agent b; < 0 or >= B: none, a disc of radius 0), radius [B] (of agent b as an obstacle).  A gather
        on the current stream; `out`: a table to write in place (one that is bound, say), else a new one.  Bound with
        index = arange(B) it makes the next solve "everyone avoids everyone's last plan"."""
        return self._rows_from_plans(self.lib.mpc_discs_from_plans, "discs", X, opp, radius, "radius", out)

    def _scene_args(self, B, G, radius, reach):
        G, reach = int(G), float(reach)
        self._check_scene(B, G)
        if not reach >= 0.0:
            raise ValueError("reach must be >= 0 (inf: every agent of the scene)")
        self._chk(radius, (B,), "radius")
        return G, reach

    def opponents_from_plans(self, X, G, radius, reach=float("inf")):
        """mpc_opponents_from_plans: (opp [B, NDISC] int32, clear [B, NDISC]) -- for every agent the NDISC agents of its
        scene (agents b // G == const) that come closest along everybody's plans X [B, Nst, nx] (rollout(); [B, nx]: the
        states as they are now): c(b, o) = min_k (dx dx + dy dy) - radius[o]^2, candidates c < reach^2 with every stage
        finite, the smallest in the order (c, o) first.  opp holds global agent indices, -1 for an unused slot (clear
        +inf): what discs_from_plans takes.  On the current stream."""
        X, B, Nst = self._plans(X)
        G, reach = self._scene_args(B, G, radius, reach)
        opp = torch.full((B, _lib.NDISC), -1, dtype=torch.int32, device=self.device)
        clear = torch.full((B, _lib.NDISC), float("inf"), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.mpc_opponents_from_plans(self._h, B, G, Nst, _ptr(X), _ptr(radius), reach, _ptr(opp), _ptr(clear),
                                                     self._stream()))
        return opp, clear

    def invalidate_centerline_tables(self):
        """Forget the nearest-point search tables: the next call rebuilds them for the table it is given."""
        self._cl_key, self._cl_keep = None, None

    def _empty(self, *shape, dtype=torch.float64):
        return torch.empty(*shape, dtype=dtype, device=self.device)

    # ------------------------------------------------------------------ model layer
    def rhs(self, x, u):
        """a-1: continuous dynamics f(x, u) (car_dynamics.py:93-132 / dynamics.py:144-173)."""
        B = x.shape[0]
        self._chk(x, (B, self.nx), "x"); self._chk(u, (B, 2), "u")
        dx = self._empty(B, self.nx)
        _lib.check(self.lib.mpc_rhs(self._h, B, _ptr(x), _ptr(u), _ptr(dx), self._stream()))
        return dx

    def rollout(self, x0, U):
        """a-3: X[B, Nsim, nx] = x_1..x_Nsim (car_dynamics.py:159-166); U is [B, 2*Nsim]."""
        B = x0.shape[0]
        self._chk(x0, (B, self.nx), "x0")
        if U.dim() != 2 or U.shape[0] != B or U.shape[1] % 2:
            raise ValueError("U: expected [B, 2*Nsim]")
        self._chk(U, U.shape, "U")
        Nsim = U.shape[1] // 2
        X = self._empty(B, Nsim, self.nx)
        _lib.check(self.lib.mpc_rollout(self._h, B, Nsim, _ptr(x0), _ptr(U), _ptr(X), self._stream()))
        return X

    def stage_errors(self, pose, centerline, cl_index=None):
        """a-4/a-5: (err[B,3] = [cte, heading_error, pos_error], idx[B])."""
        B = pose.shape[0]
        self._chk(pose, (B, 3), "pose")
        cl = self._centerline(centerline, cl_index, B)
        err = self._empty(B, 3)
        idx = self._empty(B, dtype=torch.int32)
        _lib.check(self.lib.mpc_stage_errors(self._h, B, _ptr(pose), _ptr(cl), _ptr(cl_index),
                                             _ptr(err), _ptr(idx), self._stream()))
        return err, idx

    def stage_cost(self, x, u, centerline, cl_index=None):
        """a-6: L[B] (car_dynamics.py:252-258)."""
        B = x.shape[0]
        self._chk(x, (B, self.nx), "x"); self._chk(u, (B, 2), "u")
        cl = self._centerline(centerline, cl_index, B)
        out = self._empty(B)
        _lib.check(self.lib.mpc_stage_cost(self._h, B, _ptr(x), _ptr(u), _ptr(cl), _ptr(cl_index),
                                           _ptr(out), self._stream()))
        return out

    def eval_cost_grad(self, x0, centerline, U, y=None, Sigma=None, cl_index=None, want_grad=True, wave=False):
        """K1: psi[B], grad[B, 2N] (or None), yhat[B, m] (or None).  wave=True: the wave-per-agent
        evaluation of the persistent solve kernel instead of the K1a/K1b/K1c launches (same bits)."""
        B = x0.shape[0]
        self._chk(x0, (B, self.nx), "x0"); self._chk(U, (B, self.n), "U")
        cl = self._centerline(centerline, cl_index, B)
        if self.m:
            if y is None or Sigma is None:
                raise ValueError("y and Sigma are required when the problem has constraints")
            self._chk(y, (B, self.m), "y"); self._chk(Sigma, (B, self.m), "Sigma")
        psi = self._empty(B)
        grad = self._empty(B, self.n) if want_grad else None
        yhat = self._empty(B, self.m) if self.m else None
        fn = self.lib.mpc_eval_cost_grad_wave if wave else self.lib.mpc_eval_cost_grad
        _lib.check(fn(self._h, B, _ptr(x0), _ptr(cl), _ptr(cl_index), _ptr(U), _ptr(y), _ptr(Sigma), _ptr(psi),
                      _ptr(grad), _ptr(yhat), self._stream()))
        return psi, grad, yhat

    def eval_cost_grad_pair(self, x0, centerline, U, U2, y=None, Sigma=None, cl_index=None, want_grad=True):
        """K1 at two points of every agent in one trip of the wave-per-agent evaluation: psi[B], grad[B, 2N] (or None)
        and yhat[B, m] (or None) at U, and grad2[B, 2N] at U2 -- the request and the speculative gradient of a trip of
        the kinematic persistent kernel (nfe = 4, N <= 32).  Same bits as two calls of eval_cost_grad."""
        B = x0.shape[0]
        self._chk(x0, (B, self.nx), "x0"); self._chk(U, (B, self.n), "U"); self._chk(U2, (B, self.n), "U2")
        cl = self._centerline(centerline, cl_index, B)
        if self.m:
            if y is None or Sigma is None:
                raise ValueError("y and Sigma are required when the problem has constraints")
            self._chk(y, (B, self.m), "y"); self._chk(Sigma, (B, self.m), "Sigma")
        psi = self._empty(B)
        grad = self._empty(B, self.n) if want_grad else None
        grad2 = self._empty(B, self.n)
        yhat = self._empty(B, self.m) if self.m else None
        _lib.check(self.lib.mpc_eval_cost_grad_wave2(self._h, B, _ptr(x0), _ptr(cl), _ptr(cl_index), _ptr(U), _ptr(U2), _ptr(y),
                                                     _ptr(Sigma), _ptr(psi), _ptr(grad), _ptr(grad2), _ptr(yhat), self._stream()))
        return psi, grad, grad2, yhat

    # ------------------------------------------------------------------ solver pieces
    def prox_step(self, x, grad, gamma):
        """K2: xhat, p, [||p||^2, grad'p]."""
        B = x.shape[0]
        self._chk(x, (B, self.n), "x"); self._chk(grad, (B, self.n), "grad"); self._chk(gamma, (B,), "gamma")
        xhat, p, out = self._empty(B, self.n), self._empty(B, self.n), self._empty(B, 2)
        _lib.check(self.lib.mpc_prox_step(self._h, B, _ptr(x), _ptr(grad), _ptr(gamma), _ptr(xhat),
                                          _ptr(p), _ptr(out), self._stream()))
        return xhat, p, out

    def lbfgs_apply(self, S, Y, idx, full, mask, q):
        """K3: masked two-loop on q (copied); returns (q_out, ok)."""
        B = q.shape[0]
        self._chk(S, (B, self.M, self.n), "S"); self._chk(Y, (B, self.M, self.n), "Y")
        self._chk(idx, (B,), "idx", torch.int32); self._chk(full, (B,), "full", torch.int32)
        self._chk(mask, (B, self.n), "mask"); self._chk(q, (B, self.n), "q")
        if B and (int(idx.min()) < 0 or int(idx.max()) >= self.M):
            raise ValueError("idx out of range")
        qo = q.clone()
        ok = self._empty(B, dtype=torch.int32)
        _lib.check(self.lib.mpc_lbfgs_apply(self._h, B, _ptr(S), _ptr(Y), _ptr(idx), _ptr(full), _ptr(mask),
                                            _ptr(qo), _ptr(ok), self._stream()))
        return qo, ok

    # ------------------------------------------------------------------ the solve
    def solve(self, x0, centerline, U, lam=None, cl_index=None, inplace=False):
        """a-8..a-13: returns (U*, lambda*, stats[B, 8]); warm start from U / lam."""
        B = x0.shape[0]
        self._chk(x0, (B, self.nx), "x0"); self._chk(U, (B, self.n), "U")
        cl = self._centerline(centerline, cl_index, B)
        if not inplace:
            U = U.clone()
        lam = self._multipliers(B, lam, inplace)
        stats = self._empty(B, _lib.NSTATS)
        _lib.check(self.lib.mpc_solve_batch(self._h, B, _ptr(x0), _ptr(cl), _ptr(cl_index), _ptr(U),
                                            _ptr(lam), _ptr(stats), self._stream()))
        return U, lam, stats

    def solve_async(self, x0, centerline, U, lam=None, cl_index=None):
        """The same solve without holding the caller's thread (mpc_solve_batch_async): returns a function;
        calling it waits for the solve (mpc_solve_wait) and returns (U*, lambda*, stats).  One solve in
        flight per engine; no other call on the engine in between."""
        self._free()
        B = x0.shape[0]
        self._chk(x0, (B, self.nx), "x0"); self._chk(U, (B, self.n), "U")
        cl = self._centerline(centerline, cl_index, B)
        U = U.clone()
        lam = self._multipliers(B, lam)
        stats = self._empty(B, _lib.NSTATS)
        keep = (x0, cl, cl_index, U, lam, stats)      # the buffers stay alive until the wait
        _lib.check(self.lib.mpc_solve_batch_async(self._h, B, _ptr(x0), _ptr(cl), _ptr(cl_index), _ptr(U),
                                                  _ptr(lam), _ptr(stats), self._stream()))
        self._pending = True

        def wait():
            try:
                _lib.check(self.lib.mpc_solve_wait(self._h))
            finally:
                self._pending = False
            return keep[3], keep[4], keep[5]
        return wait

    def closed_loop(self, x, centerline, U, T, lam=None, cl_index=None, shift=False):
        """f-1 (main.py:121-146) for B agents: returns (x_T, U, lam, traj_x[B,T,nx], traj_u[B,T,2],
        failures[B], stats of the last solve)."""
        B = self._loop_entry(x, U)
        cl = self._centerline(centerline, cl_index, B)
        x, U, lam, tx, tu, fails, stats = self._loop_state(B, T, x, U, lam)
        _lib.check(self.lib.mpc_closed_loop(self._h, B, int(T), int(bool(shift)), _ptr(x), _ptr(cl),
                                            _ptr(cl_index), _ptr(U), _ptr(lam), _ptr(tx), _ptr(tu),
                                            _ptr(fails), _ptr(stats), self._stream()))
        return x, U, lam, tx, tu, fails, stats

    def closed_loop_traffic(self, x, centerline, U, T, G, radius, reach=float("inf"), lam=None, cl_index=None, shift=False,
                            table=None):
        """mpc_closed_loop_traffic (an engine of CONSTR_DISCS): closed_loop in which, at every step, every agent avoids
        the current plans of the NDISC nearest agents of its scene (opponents_from_plans on rollout(x, U), then
        discs_from_plans into the bound table, then the solve and the plant step).  radius [B]: of agent b as an
        obstacle.  table: the bound disc table [B, 3 NDISC N] (set_agent_discs with index = arange(B)), rewritten in
        place; None: a table of zeros is made, bound with arange(B) and left bound.  Returns a TrafficLoopResult (x, U
        and lam are copies; the table is the bound one)."""
        B, T = self._loop_entry(x, U), int(T)
        if T < 0:
            raise ValueError("T must be >= 0")
        G, reach = self._scene_args(B, G, radius, reach)
        if int(self.cfg.constr_mode) != _lib.CONSTR_DISCS:     # before a table is made and bound for the caller
            raise _lib.MpcError("libmpc_hip error -1: mpc_closed_loop_traffic: the handle's constr_mode is not MPC_CONSTR_DISCS")
        table = self._loop_table("discs", B, table)
        cl = self._centerline(centerline, cl_index, B)
        x, U, lam, tx, tu, fails, stats = self._loop_state(B, T, x, U, lam)    # (an engine of CONSTR_DISCS has m > 0)
        topp = torch.full((B, T, _lib.NDISC), -1, dtype=torch.int32, device=self.device)
        tclear = torch.full((B, T), float("inf"), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.mpc_closed_loop_traffic(
            self._h, B, T, int(bool(shift)), G, _ptr(radius), reach, _ptr(x), _ptr(cl), _ptr(cl_index), _ptr(U), _ptr(lam),
            _ptr(table), _ptr(tx), _ptr(tu), _ptr(topp), _ptr(tclear), _ptr(fails), _ptr(stats), self._stream()))
        return TrafficLoopResult(x, U, lam, tx, tu, fails, stats, topp, tclear, table)

    def closed_loop_traffic_field(self, x, centerline, U, T, G, radius, shape, reach=float("inf"), lam=None, cl_index=None,
                                  shift=False, table=None):
        """mpc_closed_loop_traffic_field (an engine of any constr_mode but CONSTR_DISCS): closed_loop_traffic with soft
        obstacles -- at every step every agent's cost gets the risk fields of the current plans of the NFIELD nearest
        agents of its scene (opponents_from_plans on rollout(x, U), then fields_from_plans into the bound table, then the
        solve and the plant step).  radius [B] drives the selection and traj_clear, shape [B, 4] = [A, kx, ky, gain] is
        agent b as an obstacle.  table: the bound field table [B, NFIELD NFSRC N] (set_agent_fields with index =
        arange(B)), rewritten in place; None: a table of zeros is made, bound with arange(B) and left bound.  Returns a
        TrafficLoopResult (x, U and lam are copies, lam None where the engine has no constraints; the table is the bound
        one)."""
        B, T = self._loop_entry(x, U), int(T)
        if T < 0:
            raise ValueError("T must be >= 0")
        G, reach = self._scene_args(B, G, radius, reach)
        self._chk(shape, (B, 4), "shape")
        if int(self.cfg.constr_mode) == _lib.CONSTR_DISCS:     # before a table is made and bound for the caller
            raise ValueError("closed_loop_traffic_field: the engine's constr_mode is CONSTR_DISCS, where an obstacle is a disc "
                             "(closed_loop_traffic)")
        table = self._loop_table("fields", B, table)
        cl = self._centerline(centerline, cl_index, B)
        x, U, lam, tx, tu, fails, stats = self._loop_state(B, T, x, U, lam)
        topp = torch.full((B, T, _lib.NFIELD), -1, dtype=torch.int32, device=self.device)
        tclear = torch.full((B, T), float("inf"), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.mpc_closed_loop_traffic_field(
            self._h, B, T, int(bool(shift)), G, _ptr(radius), _ptr(shape), reach, _ptr(x), _ptr(cl), _ptr(cl_index), _ptr(U),
            _ptr(lam), _ptr(table), _ptr(tx), _ptr(tu), _ptr(topp), _ptr(tclear), _ptr(fails), _ptr(stats), self._stream()))
        return TrafficLoopResult(x, U, lam, tx, tu, fails, stats, topp, tclear, table)

    # ------------------------------------------------------------------ masked solve, event-triggered loop
    def _weights(self, w):
        w = [float(v) for v in (w.tolist() if hasattr(w, "tolist") else w)]
        if len(w) != self.nx:
            raise ValueError(f"w: expected {self.nx} weights, got {len(w)}")
        return (C.c_double * self.nx)(*w)

    def _trigger_args(self, thr, max_hold):
        thr, max_hold = float(thr), int(max_hold)
        if not thr >= 0.0:
            raise ValueError("thr must be >= 0 (inf: the hold limit alone)")
        if not 1 <= max_hold <= self.N:
            raise ValueError(f"max_hold must be in [1, {self.N}]")
        return thr, max_hold

    def solve_active(self, x0, centerline, U, active, lam=None, cl_index=None, stats=None, inplace=False):
        """mpc_solve_active: solves the agents with active[b] != 0 (int32 or bool [B]) exactly as solve() would and
        leaves every other agent's rows of U, lam and stats as they are.  Returns (U, lam, stats, n_active); the
        tensors are copies unless inplace (stats=None: zeros for the agents that are not solved)."""
        B = x0.shape[0]
        self._chk(x0, (B, self.nx), "x0"); self._chk(U, (B, self.n), "U")
        if isinstance(active, torch.Tensor) and active.dtype == torch.bool:
            active = active.to(torch.int32)
        self._chk(active, (B,), "active", torch.int32)
        cl = self._centerline(centerline, cl_index, B)
        if not inplace:
            U = U.clone()
        lam = self._multipliers(B, lam, inplace)
        if stats is None:
            stats = torch.zeros(B, _lib.NSTATS, dtype=torch.float64, device=self.device)
        elif not inplace:
            stats = stats.clone()
        self._chk(stats, (B, _lib.NSTATS), "stats")
        n = C.c_int32(0)
        _lib.check(self.lib.mpc_solve_active(self._h, B, _ptr(active), _ptr(x0), _ptr(cl), _ptr(cl_index), _ptr(U),
                                             _ptr(lam), _ptr(stats), C.byref(n), self._stream()))
        return U, lam, stats, int(n.value)

    def trigger_eval(self, x, xhat, held, w, thr, max_hold):
        """mpc_trigger_eval: (dev2 [B], fire [B] int32) with e = x - xhat (heading reduced by whole turns),
        dev2 = sum_i w_i e_i^2, fire = held < 0 or held >= max_hold or dev2 >= thr^2.  w: nx host floats."""
        self._free()
        B = x.shape[0]
        self._chk(x, (B, self.nx), "x"); self._chk(xhat, (B, self.nx), "xhat")
        self._chk(held, (B,), "held", torch.int32)
        thr, max_hold = self._trigger_args(thr, max_hold)
        dev2 = self._empty(B)
        fire = self._empty(B, dtype=torch.int32)
        _lib.check(self.lib.mpc_trigger_eval(self._h, B, _ptr(x), _ptr(xhat), _ptr(held), self._weights(w), thr, max_hold,
                                             _ptr(dev2), _ptr(fire), self._stream()))
        return dev2, fire

    def closed_loop_event(self, x, centerline, U, T, w, thr, max_hold, held=None, lam=None, cl_index=None,
                          shift=False, disturbance=None, stats=None):
        """mpc_closed_loop_event for B agents: T steps in which an agent is solved again only when its state has left
        the plan's own prediction by thr (weights w, heading by whole turns) or max_hold stages of the plan have been
        applied.  held [B] int32 (None: -1, no plan yet) and the returned U / held / lam / stats continue a loop
        on this engine: pass them to the next call.  disturbance [B, T, nx] is added to the plant's state at every
        step.  Returns an EventLoopResult (copies; the arguments are not written)."""
        B, T = self._loop_entry(x, U), int(T)
        thr, max_hold = self._trigger_args(thr, max_hold)
        if T < 0:
            raise ValueError("T must be >= 0")
        cl = self._centerline(centerline, cl_index, B)
        res = EventLoopResult(*self._event_loop_state(B, T, x, U, lam, held, disturbance, stats))
        _lib.check(self.lib.mpc_closed_loop_event(
            self._h, B, T, int(bool(shift)), self._weights(w), thr, max_hold, _ptr(res.x), _ptr(cl), _ptr(cl_index), _ptr(res.U),
            _ptr(res.lam), _ptr(res.held), _ptr(disturbance), _ptr(res.traj_x), _ptr(res.traj_u), _ptr(res.solved),
            _ptr(res.solve_count), _ptr(res.failures), _ptr(res.stats), self._stream()))
        return res

    # ------------------------------------------------------------------ lap driving: windows of a track
    def track_windows(self, track, stride, lead, closed):
        """mpc_track_init + mpc_track_windows: cuts `track` [K, 2L] (or [2L]: one track; rows flat x.. then y.., a closed
        track without a repeated closing point) into windows of S points every `stride` points and returns the Track
        that holds them.  The nearest-point tables for the window table are prepared here, once (not for more than
        1 024 windows: such a table takes the full scan -- the same results, slower)."""
        self._free()
        if isinstance(track, torch.Tensor) and track.dim() == 1:
            track = track.unsqueeze(0)
        if not isinstance(track, torch.Tensor) or track.dim() != 2 or track.shape[1] % 2:
            raise ValueError("track: expected a tensor [K, 2L] (flat x.. then y..)")
        self._chk(track, track.shape, "track")
        K, L = int(track.shape[0]), int(track.shape[1]) // 2
        geom = _lib.track_init(self.cfg, K, L, stride, lead, closed)
        win = self._empty(K * int(geom.R), 2 * self.S)
        _lib.check(self.lib.mpc_track_windows(self._h, C.byref(geom), _ptr(track), _ptr(win), self._stream()))
        trk = Track(geom, self.S, track, win)
        self._centerline(win, None, 0)
        return trk

    def _track(self, trk):
        if not isinstance(trk, Track):
            raise TypeError("expected the Track that track_windows returned")
        if trk.S != self.S or trk.win.device != self.device:
            raise ValueError("this Track was made by another engine (other S or device)")
        return trk

    def _pose(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            raise ValueError(f"x: expected [B, {self.nx}]")
        B = x.shape[0]
        self._chk(x, (B, self.nx), "x")
        return B

    def track_locate(self, x, track_obj, track_index=None):
        """mpc_track_locate: the first placement -- cl_index [B] int32, each agent's row of track_obj.win, from the
        nearest point of its whole track (track_index [B] int32, None: track 0) to x[b, :2]."""
        self._free()
        trk, B = self._track(track_obj), self._pose(x)
        if track_index is not None:
            self._chk(track_index, (B,), "track_index", torch.int32)
            if B and (int(track_index.min()) < 0 or int(track_index.max()) >= trk.K):
                raise ValueError("track_index out of range")
        ci = torch.zeros(B, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.mpc_track_locate(self._h, C.byref(trk._c), B, _ptr(x), _ptr(trk.track), _ptr(track_index),
                                             _ptr(ci), self._stream()))
        return ci

    def track_select(self, x, track_obj, cl_index, active=None):
        """mpc_track_select: (cl_index [B] int32, pos [B] int32) -- the rows after re-selection from x[b, :2] and the
        track point each agent stands at.  Agents with active[b] == 0 (int32 or bool [B]; None: all active) and agents
        whose x or y is not finite keep their row; their pos is -1.  Returns copies."""
        trk, B = self._track(track_obj), self._pose(x)
        win = self._centerline(trk.win, cl_index, B)
        if isinstance(active, torch.Tensor) and active.dtype == torch.bool:
            active = active.to(torch.int32)
        if active is not None:
            self._chk(active, (B,), "active", torch.int32)
        ci = cl_index.clone()
        pos = torch.full((B,), -1, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.mpc_track_select(self._h, C.byref(trk._c), B, _ptr(x), _ptr(win), _ptr(active), _ptr(ci),
                                             _ptr(pos), self._stream()))
        return ci, pos

    def closed_loop_track(self, x, track_obj, U, T, w, thr, max_hold, cl_index, held=None, lam=None, shift=False,
                          disturbance=None, stats=None):
        """mpc_closed_loop_track: closed_loop_event on the windows of a track -- at every step the agents that re-plan
        first re-select their row of track_obj.win from the plant state; an agent that holds its plan keeps the row the
        plan was solved on.  cl_index [B] int32: the rows to start from (track_locate; or the cl_index of an earlier
        result, with its U / held / lam / stats, to continue).  Returns a TrackLoopResult (copies; the arguments are
        not written)."""
        trk = self._track(track_obj)
        B, T = self._loop_entry(x, U), int(T)
        thr, max_hold = self._trigger_args(thr, max_hold)
        if T < 0:
            raise ValueError("T must be >= 0")
        if cl_index is None:
            raise ValueError("cl_index: the rows to start from are required (track_locate)")
        win = self._centerline(trk.win, cl_index, B)
        res = TrackLoopResult(*self._event_loop_state(B, T, x, U, lam, held, disturbance, stats), cl_index.clone(),
                              torch.zeros(B, T, dtype=torch.int32, device=self.device))
        _lib.check(self.lib.mpc_closed_loop_track(
            self._h, B, T, int(bool(shift)), self._weights(w), thr, max_hold, _ptr(res.x), _ptr(win), _ptr(res.cl_index), _ptr(res.U),
            _ptr(res.lam), _ptr(res.held), _ptr(disturbance), _ptr(res.traj_x), _ptr(res.traj_u), _ptr(res.solved),
            _ptr(res.solve_count), _ptr(res.failures), _ptr(res.stats), self._stream(), C.byref(trk._c), _ptr(res.traj_row)))
        return res

    # ------------------------------------------------------------------ scripted obstacles
    def _obstacle_args(self, B, G, obs, wrap, ti, Nst, reach=0.0):
        """(G, K, Lt, wrap, ti, reach) of a call on the obstacle tracks obs [B / G, K, Lt, W]"""
        G, ti, reach = int(G), int(ti), float(reach)
        self._check_scene(B, G)
        W = _lib.obstacle_width(self.cfg)
        if not isinstance(obs, torch.Tensor) or obs.dim() != 4 or obs.shape[3] != W:
            raise ValueError(f"obs: expected a tensor [B / G, K, Lt, {W}]")
        K, Lt = int(obs.shape[1]), int(obs.shape[2])
        if not 1 <= K <= _lib.SCENE_MAX or Lt < 1:
            raise ValueError(f"obs: a scene has 1 .. {_lib.SCENE_MAX} obstacles of Lt >= 1 samples, got K = {K}, Lt = {Lt}")
        self._chk(obs, (B // G, K, Lt, W), "obs")
        if ti < 0 or ti + int(Nst) > 2 ** 31 - 1:
            raise ValueError("the window of samples must start at a time >= 0 and end within an int32")
        if not reach >= 0.0:
            raise ValueError("reach must be >= 0 (inf: every obstacle of the scene)")
        return G, K, Lt, int(bool(wrap)), ti, reach

    def obstacles_select(self, X, G, obs, ti=0, reach=float("inf"), wrap=False):
        """mpc_obstacles_select: (sel [B, NDISC] int32, clear [B, NDISC]) -- for every agent the NDISC scripted obstacles of
        its scene (obs [B / G, K, Lt, W], _lib.obstacle_tracks) that come closest along the plans X [B, Nst, nx] (rollout();
        [B, nx]: the states as they are now), stage k against sample ti + k (wrap: i mod Lt, else the last sample stands):
        c(b, o) = min over the present samples of (dx dx + dy dy) - r^2 (fields: r = 0), candidates c < reach^2 with every
        stage finite, the smallest in the order (c, o) first.  sel holds indices within the scene, -1 for an unused slot
        (clear +inf): what discs_from_obstacles / fields_from_obstacles take.  On the current stream."""
        X, B, Nst = self._plans(X)
        G, K, Lt, wrap, ti, reach = self._obstacle_args(B, G, obs, wrap, ti, Nst, reach)
        sel = torch.full((B, _lib.NDISC), -1, dtype=torch.int32, device=self.device)
        clear = torch.full((B, _lib.NDISC), float("inf"), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.mpc_obstacles_select(self._h, B, G, K, Lt, wrap, ti, Nst, _ptr(X), _ptr(obs), reach, _ptr(sel),
                                                 _ptr(clear), self._stream()))
        return sel, clear

    def _rows_from_obstacles(self, fn, width, sel, G, obs, ti, wrap, out):
        self._free()
        if not isinstance(sel, torch.Tensor) or sel.dim() != 2:
            raise ValueError(f"sel: expected [B, {_lib.NDISC}] int32")
        B = int(sel.shape[0])
        self._chk(sel, (B, _lib.NDISC), "sel", torch.int32)
        G, K, Lt, wrap, ti, _ = self._obstacle_args(B, G, obs, wrap, ti, self.N)
        table = self._empty(B, width) if out is None else self._chk(out, (B, width), "out")
        _lib.check(fn(self._h, B, G, K, Lt, wrap, ti, _ptr(obs), _ptr(sel), _ptr(table), self._stream()))
        return table

    def discs_from_obstacles(self, sel, G, obs, ti=0, wrap=False, out=None):
        """mpc_discs_from_obstacles (an engine of CONSTR_DISCS): the disc table [B, 3 NDISC N] whose entry (k, j) of agent b
        is sample ti + k of obstacle sel[b, j] of b's scene, zeros where sel is -1 (or outside [0, K)) or the sample is
        absent (r == 0).  A gather on the current stream; `out`: a table to write in place, else a new one."""
        if int(self.cfg.constr_mode) != _lib.CONSTR_DISCS:
            raise _lib.MpcError("libmpc_hip error -1: mpc_discs_from_obstacles: the handle's constr_mode is not MPC_CONSTR_DISCS")
        return self._rows_from_obstacles(self.lib.mpc_discs_from_obstacles, 3 * _lib.NDISC * self.N, sel, G, obs, ti, wrap, out)

    def fields_from_obstacles(self, sel, G, obs, ti=0, wrap=False, out=None):
        """mpc_fields_from_obstacles (an engine of any constr_mode but CONSTR_DISCS): the field table [B, NFIELD NFSRC N]
        whose entry (k, j) of agent b is sample ti + k of obstacle sel[b, j] of b's scene, zeros where sel is -1 (or
        outside [0, K)) or the sample is absent (A == 0).  `out`: a table to write in place, else a new one."""
        if int(self.cfg.constr_mode) == _lib.CONSTR_DISCS:
            raise _lib.MpcError("libmpc_hip error -1: mpc_fields_from_obstacles: the handle's constraints are keep-out discs "
                                "(constr_mode MPC_CONSTR_DISCS): there an obstacle is a disc (mpc_set_agent_discs)")
        return self._rows_from_obstacles(self.lib.mpc_fields_from_obstacles, _lib.field_row(self.N), sel, G, obs, ti, wrap, out)

    def closed_loop_obstacles(self, x, centerline, U, T, G, obs, reach=float("inf"), t0=0, wrap=False, lam=None, cl_index=None,
                              shift=False, table=None, track_obj=None):
        """mpc_closed_loop_obstacles: closed_loop among scripted moving obstacles -- at every step every agent avoids the
        NDISC obstacles of its scene (obs [B / G, K, Lt, W], _lib.obstacle_tracks) that come closest to its current plan,
        stage k of the re-plan of step t reading sample t0 + t + 1 + k of their scripts (obstacles_select on rollout(x, U),
        then discs_from_obstacles -- an engine of CONSTR_DISCS -- or fields_from_obstacles into the bound table, then the
        solve and the plant step).  table: the bound disc / field table with index = arange(B), rewritten in place; None:
        a table of zeros is made, bound with arange(B) and left bound.  track_obj: a Track (track_windows) -- the
        centerline is its window table (pass centerline=None) and every agent re-selects its row cl_index [B] (required:
        track_locate) from its state before every step.  t0: the script's time at the call (a second call with t0 + T,
        and x, U, lam, cl_index of the first's result, continues it).  Returns an ObstacleLoopResult (copies; the table is
        the bound one)."""
        B, T, t0 = self._loop_entry(x, U), int(T), int(t0)
        if T < 0:
            raise ValueError("T must be >= 0")
        G, K, Lt, wrap, t0, reach = self._obstacle_args(B, G, obs, wrap, t0, T + self.N, reach)
        kind = "discs" if int(self.cfg.constr_mode) == _lib.CONSTR_DISCS else "fields"
        table = self._loop_table(kind, B, table, identity_index=True)
        trk = None
        if track_obj is not None:
            trk = self._track(track_obj)
            if centerline is not None and centerline is not trk.win:
                raise ValueError("with track_obj the centerline table is track_obj.win (pass centerline=None)")
            if cl_index is None:
                raise ValueError("cl_index: the rows to start from are required with track_obj (track_locate)")
            centerline = trk.win
        cl = self._centerline(centerline, cl_index, B)
        x, U, lam, tx, tu, fails, stats = self._loop_state(B, T, x, U, lam)
        ci = None if cl_index is None else cl_index.clone()
        tsel = torch.full((B, T, _lib.NDISC), -1, dtype=torch.int32, device=self.device)
        tclear = torch.full((B, T), float("inf"), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.mpc_closed_loop_obstacles(
            self._h, B, T, int(bool(shift)), G, K, Lt, wrap, t0, _ptr(obs), reach, _ptr(x), _ptr(cl), _ptr(ci), _ptr(U), _ptr(lam),
            _ptr(table), _ptr(tx), _ptr(tu), _ptr(tsel), _ptr(tclear), _ptr(fails), _ptr(stats), self._stream(),
            C.byref(trk._c) if trk is not None else None))
        return ObstacleLoopResult(x, U, lam, tx, tu, fails, stats, tsel, tclear, table, ci)

    # ------------------------------------------------------------------ event-triggered holding among scripted obstacles
    def rollout_held(self, x, U, held):
        """mpc_rollout_held: X [B, N, nx], the states an agent reaches by going on applying the plan U [B, 2N] of which it
        has applied held[b] stages (int32 [B]) -- stage j applies u_{min(k + j, N - 1)} with k = min(max(held[b], 0), N - 1),
        the last input repeated into the tail.  Bit for bit rollout(x, U shifted by k stages); held <= 0 is rollout(x, U)."""
        self._free()
        B = x.shape[0]
        self._chk(x, (B, self.nx), "x"); self._chk(U, (B, self.n), "U")
        self._chk(held, (B,), "held", torch.int32)
        X = self._empty(B, self.N, self.nx)
        _lib.check(self.lib.mpc_rollout_held(self._h, B, _ptr(x), _ptr(U), _ptr(held), _ptr(X), self._stream()))
        return X

    def obstacle_trigger(self, X, held, sel_plan, G, obs, ti=0, reach=float("inf"), clear_thr=0.0, watch=3, fire=None,
                         wrap=False):
        """mpc_obstacle_trigger: the obstacle rule of the event-triggered loop, pure.  X [B, N, nx] is rollout_held(x, U,
        held): stage j of what agent b will go on applying meets sample ti + j of the scripts.  The selection of
        obstacles_select runs over the N - k stages the held plan still has (k = min(max(held[b], 0), N - 1); the
        repeated tail is not looked at) and gives sel_chk [B, NDISC] int32 and clear_chk [B, NDISC].  why [B] uint8: bit 0
        = fire[b] != 0 (the caller's, e.g. trigger_eval's; None: zeros); for agents with held > 0, bit 1 (watch & 1) =
        not clear_chk[b, 0] >= clear_thr, bit 2 (watch & 2) = some sel_chk[b, j] >= 0 is not in the set
        sel_plan[b] ([B, NDISC] int32: the obstacles the held plan was solved against, -1: none).  clear_thr is in the
        units of the clearance: d^2 - r^2 on an engine of CONSTR_DISCS -- a solved plan rides 0 to within alm_delta, so a
        useful threshold is slightly negative --, a squared distance on every other.  Returns (fire_out = why != 0 as
        int32 [B], why, sel_chk, clear_chk)."""
        X, B, Nst = self._plans(X)
        self._chk(X, (B, self.N, self.nx), "X")
        G, K, Lt, wrap, ti, reach = self._obstacle_args(B, G, obs, wrap, ti, self.N, reach)
        clear_thr, watch = float(clear_thr), int(watch)      # (the library refuses clear_thr > reach^2 or NaN, watch outside [0, 3])
        self._chk(held, (B,), "held", torch.int32)
        self._chk(sel_plan, (B, _lib.NDISC), "sel_plan", torch.int32)
        if fire is not None:
            self._chk(fire, (B,), "fire", torch.int32)
        sel = torch.full((B, _lib.NDISC), -1, dtype=torch.int32, device=self.device)
        clear = torch.full((B, _lib.NDISC), float("inf"), dtype=torch.float64, device=self.device)
        why = torch.zeros(B, dtype=torch.uint8, device=self.device)
        out = torch.zeros(B, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.mpc_obstacle_trigger(self._h, B, G, K, Lt, wrap, ti, _ptr(X), _ptr(obs), reach, _ptr(held),
                                                 _ptr(sel_plan), clear_thr, watch, _ptr(fire), _ptr(sel), _ptr(clear), _ptr(why),
                                                 _ptr(out), self._stream()))
        return out, why, sel, clear

    def closed_loop_obstacles_event(self, x, centerline, U, T, G, obs, w, thr, max_hold, reach=float("inf"), clear_thr=0.0,
                                    watch=3, t0=0, wrap=False, held=None, sel_plan=None, lam=None, cl_index=None, shift=False,
                                    table=None, track_obj=None, disturbance=None, stats=None):
        """mpc_closed_loop_obstacles_event: closed_loop_obstacles in which an agent keeps applying the plan it holds, as in
        closed_loop_event, and re-plans when the car trigger fires (w, thr, max_hold), when the plan it would go on applying
        comes closer than clear_thr to a scripted obstacle (watch & 1) or when an obstacle that the plan was not solved
        against enters its selection (watch & 2) -- obstacle_trigger on rollout_held, stage held + k of the held plan
        meeting sample t0 + t + 1 + k.  Only the agents that re-plan get new rows of the bound disc / field table.  held
        [B] int32 (None: -1) and sel_plan [B, NDISC] int32 (None: -1) continue a loop together with the U / lam / stats /
        cl_index of an earlier result and t0 + T.  The other arguments are closed_loop_obstacles' and closed_loop_event's.
        Returns an ObstacleEventLoopResult (copies; the table is the bound one)."""
        B, T, t0 = self._loop_entry(x, U), int(T), int(t0)
        thr, max_hold = self._trigger_args(thr, max_hold)
        if T < 0:
            raise ValueError("T must be >= 0")
        G, K, Lt, wrap, t0, reach = self._obstacle_args(B, G, obs, wrap, t0, T + self.N, reach)
        clear_thr, watch = float(clear_thr), int(watch)      # (the library refuses clear_thr > reach^2 or NaN, watch outside [0, 3])
        kind = "discs" if int(self.cfg.constr_mode) == _lib.CONSTR_DISCS else "fields"
        table = self._loop_table(kind, B, table, identity_index=True)
        trk = None
        if track_obj is not None:
            trk = self._track(track_obj)
            if centerline is not None and centerline is not trk.win:
                raise ValueError("with track_obj the centerline table is track_obj.win (pass centerline=None)")
            if cl_index is None:
                raise ValueError("cl_index: the rows to start from are required with track_obj (track_locate)")
            centerline = trk.win
        cl = self._centerline(centerline, cl_index, B)
        x, U, lam, held, tx, tu, solved, count, fails, stats = self._event_loop_state(B, T, x, U, lam, held, disturbance, stats)
        sel_plan = torch.full((B, _lib.NDISC), -1, dtype=torch.int32, device=self.device) if sel_plan is None else sel_plan.clone()
        self._chk(sel_plan, (B, _lib.NDISC), "sel_plan", torch.int32)
        ci = None if cl_index is None else cl_index.clone()
        tsel = torch.full((B, T, _lib.NDISC), -1, dtype=torch.int32, device=self.device)
        tclear = torch.full((B, T), float("inf"), dtype=torch.float64, device=self.device)
        twhy = torch.zeros(B, T, dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.mpc_closed_loop_obstacles_event(
            self._h, B, T, int(bool(shift)), self._weights(w), thr, max_hold, G, K, Lt, wrap, t0, _ptr(obs), reach, clear_thr, watch,
            _ptr(x), _ptr(cl), _ptr(ci), _ptr(U), _ptr(lam), _ptr(held), _ptr(sel_plan), _ptr(table), _ptr(disturbance), _ptr(tx),
            _ptr(tu), _ptr(tsel), _ptr(tclear), _ptr(twhy), _ptr(solved), _ptr(count), _ptr(fails), _ptr(stats), self._stream(),
            C.byref(trk._c) if trk is not None else None))
        return ObstacleEventLoopResult(x, U, lam, tx, tu, fails, stats, tsel, tclear, table, ci, solved, count, held, sel_plan, twhy)

    # ------------------------------------------------------------------ event-triggered holding in traffic
    def _opp_plan(self, B, opp_plan):
        """opp_plan [B, NDISC] int32 of the traffic rule: global agent indices in [-1, B) (-1: none)"""
        self._chk(opp_plan, (B, _lib.NDISC), "opp_plan", torch.int32)
        if B and (int(opp_plan.min()) < -1 or int(opp_plan.max()) >= B):
            raise ValueError(f"opp_plan: agent indices must be in [-1, {B}) (-1: none)")
        return opp_plan

    def opponent_trigger(self, X, held, opp_plan, G, radius, reach=float("inf"), clear_thr=0.0, watch=3, fire=None):
        """mpc_opponent_trigger: the rule of obstacle_trigger on the other agents' plans, pure.  X [B, N, nx] is
        rollout_held(x, U, held): stage j of what every agent will go on applying, at time now + j + 1 for the whole batch.
        The selection of opponents_from_plans runs for agent b over the N - k stages its held plan still has (k =
        min(max(held[b], 0), N - 1); the count is b's own, the opponents' positions are read as X has them) and gives
        opp_chk [B, NDISC] int32 (global agent indices) and clear_chk [B, NDISC].  why [B] uint8: bit 0 = fire[b] != 0 (the
        caller's, e.g. trigger_eval's; None: zeros); for agents with held > 0, bit 1 (watch & 1) = not clear_chk[b, 0] >=
        clear_thr, bit 2 (watch & 2) = some opp_chk[b, j] >= 0 is not in the set opp_plan[b] ([B, NDISC] int32: the agents
        the held plan was solved against, -1: none).  Returns (fire_out = why != 0 as int32 [B], why, opp_chk, clear_chk)."""
        X, B, Nst = self._plans(X)
        self._chk(X, (B, self.N, self.nx), "X")
        G, reach = self._scene_args(B, G, radius, reach)
        clear_thr, watch = float(clear_thr), int(watch)      # (the library refuses clear_thr > reach^2 or NaN, watch outside [0, 3])
        self._chk(held, (B,), "held", torch.int32)
        self._opp_plan(B, opp_plan)
        if fire is not None:
            self._chk(fire, (B,), "fire", torch.int32)
        opp = torch.full((B, _lib.NDISC), -1, dtype=torch.int32, device=self.device)
        clear = torch.full((B, _lib.NDISC), float("inf"), dtype=torch.float64, device=self.device)
        why = torch.zeros(B, dtype=torch.uint8, device=self.device)
        out = torch.zeros(B, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.mpc_opponent_trigger(self._h, B, G, _ptr(X), _ptr(radius), reach, _ptr(held), _ptr(opp_plan), clear_thr,
                                                 watch, _ptr(fire), _ptr(opp), _ptr(clear), _ptr(why), _ptr(out), self._stream()))
        return out, why, opp, clear

    def closed_loop_traffic_event(self, x, centerline, U, T, G, radius, w, thr, max_hold, shape=None, reach=float("inf"),
                                  clear_thr=0.0, watch=3, held=None, opp_plan=None, lam=None, cl_index=None, shift=False,
                                  table=None, disturbance=None, stats=None):
        """mpc_closed_loop_traffic_event: closed_loop_traffic (an engine of CONSTR_DISCS; shape=None) or
        closed_loop_traffic_field (every other engine; shape [B, 4]) in which an agent keeps applying the plan it holds, as in
        closed_loop_event, and re-plans when the car trigger fires (w, thr, max_hold), when the plan it would go on applying
        comes closer than clear_thr to what the others would go on applying (watch & 1), or when an agent that the plan was
        not solved against enters its selection (watch & 2) -- opponent_trigger on rollout_held.  Only the agents that
        re-plan get new rows of the bound disc / field table.  held [B] int32 (None: -1) and opp_plan [B, NDISC] int32
        (None: -1) continue a loop together with the U / lam / stats of an earlier result.  The other arguments are the
        traffic loops' and closed_loop_event's.  Returns a TrafficEventLoopResult (copies; the table is the bound one)."""
        B, T = self._loop_entry(x, U), int(T)
        thr, max_hold = self._trigger_args(thr, max_hold)
        if T < 0:
            raise ValueError("T must be >= 0")
        G, reach = self._scene_args(B, G, radius, reach)
        clear_thr, watch = float(clear_thr), int(watch)      # (the library refuses clear_thr > reach^2 or NaN, watch outside [0, 3])
        discs = int(self.cfg.constr_mode) == _lib.CONSTR_DISCS
        if discs and shape is not None:                        # before a table is made and bound for the caller
            raise ValueError("closed_loop_traffic_event: the engine's constr_mode is CONSTR_DISCS, where an opponent is a disc "
                             "(shape must be None)")
        if not discs:
            if shape is None:
                raise ValueError("closed_loop_traffic_event: shape [B, 4] is required on an engine whose opponents are risk fields")
            self._chk(shape, (B, 4), "shape")
        table = self._loop_table("discs" if discs else "fields", B, table, identity_index=True)
        cl = self._centerline(centerline, cl_index, B)
        x, U, lam, held, tx, tu, solved, count, fails, stats = self._event_loop_state(B, T, x, U, lam, held, disturbance, stats)
        opp_plan = torch.full((B, _lib.NDISC), -1, dtype=torch.int32, device=self.device) if opp_plan is None else opp_plan.clone()
        self._opp_plan(B, opp_plan)
        topp = torch.full((B, T, _lib.NDISC), -1, dtype=torch.int32, device=self.device)
        tclear = torch.full((B, T), float("inf"), dtype=torch.float64, device=self.device)
        twhy = torch.zeros(B, T, dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.mpc_closed_loop_traffic_event(
            self._h, B, T, int(bool(shift)), self._weights(w), thr, max_hold, G, _ptr(radius), _ptr(shape), reach, clear_thr, watch,
            _ptr(x), _ptr(cl), _ptr(cl_index), _ptr(U), _ptr(lam), _ptr(held), _ptr(opp_plan), _ptr(table), _ptr(disturbance),
            _ptr(tx), _ptr(tu), _ptr(topp), _ptr(tclear), _ptr(twhy), _ptr(solved), _ptr(count), _ptr(fails), _ptr(stats),
            self._stream()))
        return TrafficEventLoopResult(x, U, lam, tx, tu, fails, stats, topp, tclear, table, solved, count, held, opp_plan, twhy)

    def lane_payoff(self, ego, cars, ncars, params):
        """f-3: out[B, 2, 4] = target lane 1, 2 -> [total, safety, velocity, comfort] (game_theory.py:115-244)."""
        B = ego.shape[0]
        self._chk(ego, (B, 3), "ego")
        if cars.dim() != 3 or cars.shape[0] != B or cars.shape[2] != 3:
            raise ValueError("cars: expected [B, K, 3]")
        self._chk(cars, cars.shape, "cars"); self._chk(ncars, (B,), "ncars", torch.int32)
        K = cars.shape[1]
        if B and (int(ncars.min()) < 0 or int(ncars.max()) > K):
            raise ValueError("ncars out of range")
        pa = (C.c_double * 15)(*[float(v) for v in params])
        out = self._empty(B, 2, 4)
        _lib.check(self.lib.mpc_lane_payoff(self._h, B, K, pa, _ptr(ego), _ptr(cars), _ptr(ncars), _ptr(out),
                                            self._stream()))
        return out

    def math_probe(self, op, a, b=None):
        """Device math used by the kernels (test aid): op 0 sin, 1 cos, 2 atan, 3 atan2(a, b), 4 tan, 5 exp."""
        n = a.shape[0]
        self._chk(a, (n,), "a")
        if b is not None:
            self._chk(b, (n,), "b")
        out = self._empty(n)
        _lib.check(self.lib.mpc_math_probe(self._h, n, int(op), _ptr(a), _ptr(b), _ptr(out), self._stream()))
        return out

    def set_groups(self, groups):
        """Sub-batch pipelining over HIP streams (0 = automatic)."""
        _lib.check(self.lib.mpc_set_groups(self._h, int(groups)))

    def set_nearest_blocks(self, on=True):
        """Nearest-point search of K1b: 0 / False the full 98-candidate scan, 2 / True the grid of index
        ranges -- the same index whichever runs.  (Mode 1, the block-box search, was removed: refused.)"""
        mode = (2 if on else 0) if isinstance(on, bool) else int(on)
        _lib.check(self.lib.mpc_set_nearest_blocks(self._h, mode))
        self._nearest_blocks = mode

    def set_solo_max(self, max_requests):
        """Requests per round up to which a group finishes in the persistent wave-per-agent kernel (0 = off)."""
        _lib.check(self.lib.mpc_set_solo_max(self._h, int(max_requests)))

    def set_memo(self, on=True):
        """Failed inner solves that the outer loop backtracks over without constraints are replayed from a memo
        (default) or recomputed (False): same controls, multipliers and statistics, fewer evaluations executed."""
        _lib.check(self.lib.mpc_set_memo(self._h, int(bool(on))))

    def set_round_limit(self, rounds):
        """Test aid: cap on the rounds (persistent kernel: trips per agent) of a solve; a solve that does not
        finish inside it returns MPC_E_LIMIT.  0 = the built-in guard alone."""
        _lib.check(self.lib.mpc_set_round_limit(self._h, int(rounds)))

    def set_poll_timeout(self, seconds):
        """Wall-clock bound of a solve's host-side waits (default 300 s): a solve whose device stops answering
        raises MpcError (MPC_E_HIP) instead of blocking for ever; the device is NOT synchronised on that path."""
        _lib.check(self.lib.mpc_set_poll_timeout(self._h, float(seconds)))

    def debug_spin(self, microseconds):
        """Test aid: queue the library's idling kernel on the current stream for `microseconds`."""
        _lib.check(self.lib.mpc_debug_spin(self._h, float(microseconds), self._stream()))

    def debug_records(self, B):
        """Diagnostic: {name: array[B]} of the per-agent solver records as the last solve left them."""
        import numpy as np
        self._free()
        out = np.empty((int(B), _lib.NREC))
        _lib.check(self.lib.mpc_debug_records(self._h, int(B), C.c_void_p(out.ctypes.data)))
        names = self.lib.mpc_debug_record_names().decode().split(",")
        return {nm: out[:, i] for i, nm in enumerate(names)}

    def stream_concurrency(self):
        """(streams the HIP runtime runs side by side for this process -- 5 means five or more, measured once
        per process and device --, sub-batch groups of the last solve)."""
        self._free()
        a, b = C.c_int(), C.c_int()
        _lib.check(self.lib.mpc_stream_concurrency(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_profile(self, on=True):
        _lib.check(self.lib.mpc_set_profile(self._h, int(bool(on))))

    def last_solve_info(self):
        self._free()
        r, g, c = C.c_int64(), C.c_int64(), C.c_int64()
        e, s = C.c_double(), C.c_double()
        _lib.check(self.lib.mpc_last_solve_info(self._h, C.byref(r), C.byref(g), C.byref(c),
                                                C.byref(e), C.byref(s)))
        lm, lr = C.c_double(), C.c_int64()
        _lib.check(self.lib.mpc_last_solve_info2(self._h, C.byref(lm), C.byref(lr)))
        si, su = C.c_int64(), C.c_int64()
        _lib.check(self.lib.mpc_last_speculation(self._h, C.byref(si), C.byref(su)))
        le, lh = C.c_int64(), C.c_int64()
        _lib.check(self.lib.mpc_last_lookahead(self._h, C.byref(le), C.byref(lh)))
        km = (C.c_double * 5)()
        kl = (C.c_int64 * 5)()
        sa = C.c_int64()
        _lib.check(self.lib.mpc_last_kernel_profile(self._h, km, kl, C.byref(sa)))
        ssum, slong = C.c_double(), C.c_double()
        _lib.check(self.lib.mpc_last_solo_ms(self._h, C.byref(ssum), C.byref(slong)))
        names = ("step", "rollout", "stage", "adjoint", "solo")
        return {"kernel_ms": {k: km[i] for i, k in enumerate(names)},
                "launches": {k: int(kl[i]) for i, k in enumerate(names)}, "solo_agents": int(sa.value),
                "rounds": r.value, "evals_grad": g.value, "evals_cost": c.value,
                "eval_ms": e.value, "step_ms": s.value, "launch_pairs": int(lm.value), "lbfgs_rows": lr.value,
                "spec_issued": si.value, "spec_used": su.value, "lookahead_evals": le.value, "lookahead_hits": lh.value, "groups": self.stream_concurrency()[1],
                "solo_longest_ms": slong.value}
