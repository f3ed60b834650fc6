"""ctypes binding of libmpc_hip.so (the C-ABI declared in include/mpc_hip.h).

PyTorch is used for device memory, streams and torch.distributed only; every
kernel is hand-written HIP behind the C-ABI.  There is no CPU fallback: a
missing library or a missing GPU raises.
"""
import ctypes as C
import os
import subprocess

# The HIP runtime maps a process's streams to GPU_MAX_HW_QUEUES hardware queues (4 unless set).  A
# batched solve runs its sub-batch groups on streams of their own next to the caller's: with 8 queues
# the solver takes four groups (+3.5 % solves/s at 65 536 agents); 16 leave room for a second
# handle solving beside the first (mpc_solve_batch_async).  Read by the runtime when
# it initialises, i.e. at the first GPU call of the process: importing this package first is enough.
def _default_hw_queues():
    if "GPU_MAX_HW_QUEUES" in os.environ:
        return
    try:    # too late once the runtime is up (it has read its environment): the solver then keeps to three groups
        import torch
        if torch.cuda.is_initialized():
            return
    except Exception:
        pass
    os.environ["GPU_MAX_HW_QUEUES"] = "16"


_default_hw_queues()

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPC_LIB_PATH", os.path.join(_HERE, "libmpc_hip.so"))  # override: dev experiments
_SRC = [os.path.join(_HERE, "csrc", f) for f in ("mpc_api.hip", "mpc_arena.hpp", "mpc_handle.hpp", "mpc_launch.hpp", "mpc_rounds.hpp",
                                                  "mpc_aux.hpp", "mpc_eval.hpp", "mpc_solver.hpp", "mpc_device.hpp",
                                                  "mpc_game.hpp", "mpc_solo.hpp", "mpc_event.hpp", "mpc_track.hpp",
 "mpc_obstacles.hpp", "mpc_traffic.hpp")]
_HDR = os.path.join(os.path.dirname(_HERE), "include", "mpc_hip.h")

MODEL_KINEMATIC, MODEL_PACEJKA = 0, 1
WRAP_FLOOR, WRAP_FMOD, WRAP_IEEE = 0, 1, 2
CONSTR_NONE, CONSTR_STATE_SQ, CONSTR_LANE, CONSTR_DISCS = 0, 1, 2, 3
NSTATS = 8
ST_CONVERGED = 1

EXPORTS = [
    "mpc_default_config", "mpc_nx", "mpc_m", "mpc_create", "mpc_destroy", "mpc_last_error",
    "mpc_rhs", "mpc_rollout", "mpc_stage_errors", "mpc_stage_cost", "mpc_eval_cost_grad", "mpc_prox_step",
    "mpc_lbfgs_apply", "mpc_solve_batch", "mpc_solve_batch_async", "mpc_solve_wait", "mpc_closed_loop", "mpc_last_solve_info",
    "mpc_last_solve_info2", "mpc_math_probe", "mpc_set_groups", "mpc_last_kernel_ms", "mpc_lane_payoff",
    "mpc_set_profile", "mpc_last_speculation", "mpc_last_kernel_profile", "mpc_set_solo_max",
    "mpc_eval_cost_grad_wave", "mpc_eval_cost_grad_wave2", "mpc_centerline_blocks", "mpc_set_nearest_blocks", "mpc_set_memo",
    "mpc_set_round_limit", "mpc_stream_concurrency", "mpc_last_solo_ms",
    "mpc_set_poll_timeout", "mpc_debug_spin", "mpc_debug_records", "mpc_debug_record_names", "mpc_source_hash",
    "mpc_last_lookahead", "mpc_step_lds_plan", "mpc_default_params", "mpc_set_agent_params",
    "mpc_solve_active", "mpc_trigger_eval", "mpc_closed_loop_event",
    "mpc_default_bounds", "mpc_set_agent_bounds",
    "mpc_default_constraints", "mpc_set_agent_constraints",
    "mpc_default_discs", "mpc_set_agent_discs", "mpc_discs_from_plans",
    "mpc_default_rates", "mpc_set_agent_rates",
    "mpc_default_fields", "mpc_set_agent_fields", "mpc_fields_from_plans", "mpc_closed_loop_traffic_field",
    "mpc_default_roads", "mpc_set_agent_roads", "mpc_roads_from_script",
    "mpc_opponents_from_plans", "mpc_closed_loop_traffic",
    "mpc_obstacles_select", "mpc_discs_from_obstacles", "mpc_fields_from_obstacles", "mpc_closed_loop_obstacles",
    "mpc_rollout_held", "mpc_obstacle_trigger", "mpc_closed_loop_obstacles_event",
    "mpc_opponent_trigger", "mpc_closed_loop_traffic_event",
    "mpc_track_init", "mpc_track_windows", "mpc_track_locate", "mpc_track_select", "mpc_closed_loop_track",
]
NREC = 64
NPARAM = 31     # MPC_NPARAM: doubles per row of the per-agent parameter table
# columns of a row, by field name (include/mpc_hip.h: mpc_set_agent_params)
NBOUND = 4      # MPC_NBOUND: doubles per row of the per-agent bounds table, [u_lb[0], u_lb[1], u_ub[0], u_ub[1]]
NCONSTR = 19    # MPC_NCONSTR: doubles per row of the per-agent constraint table
NRATE = 4       # MPC_NRATE: doubles per row of the per-agent rate table, [w_d, w_delta, d_prev, delta_prev]
NFIELD = 2      # MPC_NFIELD: sources of the risk field per stage (== NDISC: one opp [B, 2] serves both)
NFSRC = 8       # MPC_NFSRC: doubles per source, [cx, cy, c, s, A, kx, ky, alpha]; a row of the field table is [N][NFIELD][NFSRC]
NROAD = 8       # MPC_NROAD: doubles per stage of the road table, [off, w_off, lo, w_lo, hi, w_hi, v_tgt, w_v]; a row is [N][NROAD]
NDISC = 2       # MPC_NDISC: keep-out discs per stage; a row of the disc table is [N][NDISC][3] = (cx, cy, r)
SCENE_MAX = 64  # MPC_SCENE_MAX: agents per scene at most (mpc_opponents_from_plans, mpc_closed_loop_traffic)
# columns of a constraint row, by field name (include/mpc_hip.h: mpc_set_agent_constraints)
CONSTR_FIELDS = {"g_off": (0, 6), "D_lb": (6, 6), "D_ub": (12, 6), "lane_halfwidth": (18, 1)}
PARAM_FIELDS = {"veh": (0, 22), "accel": (22, 1), "friction": (23, 1), "v_ref": (24, 1), "cost_w": (25, 6)}


class MpcConfig(C.Structure):
    """Mirror of `mpc_config` (include/mpc_hip.h)."""
    _fields_ = [
        ("model", C.c_int32), ("N", C.c_int32), ("S", C.c_int32), ("nfe", C.c_int32),
        ("wrap_mode", C.c_int32), ("clip_inputs", C.c_int32), ("constr_mode", C.c_int32),
        ("lbfgs_memory", C.c_int32), ("max_iter", C.c_int32), ("max_outer", C.c_int32),
        ("hess_heuristic", C.c_int32), ("max_no_progress", C.c_int32),
        ("Ts", C.c_double), ("v_ref", C.c_double), ("cost_w", C.c_double * 6),
        ("veh", C.c_double * 22), ("accel", C.c_double), ("friction", C.c_double),
        ("u_lb", C.c_double * 2), ("u_ub", C.c_double * 2), ("g_off", C.c_double * 6),
        ("D_lb", C.c_double * 6), ("D_ub", C.c_double * 6), ("lane_halfwidth", C.c_double),
        ("alm_eps", C.c_double), ("alm_delta", C.c_double), ("Sigma0", C.c_double),
        ("eps0", C.c_double), ("rho", C.c_double), ("Delta", C.c_double), ("theta", C.c_double),
        ("M", C.c_double), ("Sigma_max", C.c_double), ("Delta_lower", C.c_double),
        ("Sigma0_lower", C.c_double), ("eps0_increase", C.c_double), ("rho_increase", C.c_double),
        ("max_num_initial_retries", C.c_int32), ("max_num_retries", C.c_int32),
        ("max_total_num_retries", C.c_int32), ("max_total_inner", C.c_int32),
        ("max_total_evals", C.c_int32),
        ("lip_eps", C.c_double), ("lip_delta", C.c_double), ("Lgamma_factor", C.c_double),
        ("L_min", C.c_double), ("L_max", C.c_double), ("tau_min", C.c_double),
        ("qub_tol", C.c_double),
    ]


class MpcTrack(C.Structure):
    """Mirror of `mpc_track` (include/mpc_hip.h): the geometry of a table of track windows, filled by mpc_track_init."""
    _fields_ = [("K", C.c_int32), ("L", C.c_int32), ("stride", C.c_int32), ("lead", C.c_int32),
                ("closed", C.c_int32), ("R", C.c_int32)]


def source_hash():
    """SHA-256 over the library's sources and its header, in a fixed order: what `build()` compiles into the
    library as its identity (mpc_source_hash) and what a committed profile names as the build it measured."""
    import hashlib
    h = hashlib.sha256()
    for p in _SRC + [_HDR]:
        h.update(os.path.basename(p).encode() + b"\0")
        h.update(open(p, "rb").read())
    return h.hexdigest()


def build(force=False, verbose=False):
    """hipcc cross-compiles the library for gfx950 (works without a GPU)."""
    newest = max(os.path.getmtime(p) for p in _SRC + [_HDR])
    if not force and os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= newest:
        return LIB_PATH
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC",
           "-DMPC_SOURCE_SHA256=\"%s\"" % source_hash(), "-o", LIB_PATH, _SRC[0]]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=_HERE)
    return LIB_PATH


_lib = None


def load():
    """dlopen libmpc_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the MPC hot path has no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp, ci = C.c_void_p, C.c_int
    cp = C.POINTER(MpcConfig)
    L.mpc_default_config.argtypes = [cp, ci, ci]
    L.mpc_nx.argtypes = [cp]
    L.mpc_m.argtypes = [cp]
    L.mpc_create.argtypes = [cp, ci, C.POINTER(vp)]
    L.mpc_destroy.argtypes = [vp]
    L.mpc_last_error.restype = C.c_char_p
    L.mpc_rhs.argtypes = [vp, ci, vp, vp, vp, vp]
    L.mpc_rollout.argtypes = [vp, ci, ci, vp, vp, vp, vp]
    L.mpc_stage_errors.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]
    L.mpc_stage_cost.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]
    L.mpc_eval_cost_grad.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mpc_eval_cost_grad_wave.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mpc_eval_cost_grad_wave2.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mpc_prox_step.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp]
    L.mpc_lbfgs_apply.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mpc_solve_batch.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp]
    L.mpc_solve_batch_async.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp]
    L.mpc_solve_wait.argtypes = [vp]
    L.mpc_closed_loop.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mpc_solve_active.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_int32), vp]
    L.mpc_trigger_eval.argtypes = [vp, ci, vp, vp, vp, C.POINTER(C.c_double), C.c_double, ci, vp, vp, vp]
    L.mpc_closed_loop_event.argtypes = [vp, ci, ci, ci, C.POINTER(C.c_double), C.c_double, ci, vp, vp, vp, vp, vp, vp,
                                        vp, vp, vp, vp, vp, vp, vp, vp]
    tp = C.POINTER(MpcTrack)
    L.mpc_track_init.argtypes = [tp, cp, ci, ci, ci, ci, ci]
    L.mpc_track_windows.argtypes = [vp, tp, vp, vp, vp]
    L.mpc_track_locate.argtypes = [vp, tp, ci, vp, vp, vp, vp, vp]
    L.mpc_track_select.argtypes = [vp, tp, ci, vp, vp, vp, vp, vp, vp]
    L.mpc_closed_loop_track.argtypes = L.mpc_closed_loop_event.argtypes + [tp, vp]
    L.mpc_last_solve_info.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                      C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double)]
    L.mpc_last_solve_info2.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.mpc_last_speculation.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.mpc_last_lookahead.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.mpc_default_params.argtypes = [cp, C.POINTER(C.c_double)]
    L.mpc_set_agent_params.argtypes = [vp, vp, ci, vp, vp, ci]
    L.mpc_default_bounds.argtypes = [cp, C.POINTER(C.c_double)]
    L.mpc_set_agent_bounds.argtypes = [vp, vp, ci, vp, ci]
    L.mpc_default_constraints.argtypes = [cp, C.POINTER(C.c_double)]
    L.mpc_set_agent_constraints.argtypes = [vp, vp, ci, vp, ci]
    L.mpc_default_discs.argtypes = [cp, C.POINTER(C.c_double)]
    L.mpc_set_agent_discs.argtypes = [vp, vp, ci, vp, ci]
    L.mpc_discs_from_plans.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    L.mpc_default_rates.argtypes = [cp, C.POINTER(C.c_double)]
    L.mpc_set_agent_rates.argtypes = [vp, vp, ci, vp, ci]
    L.mpc_default_fields.argtypes = [cp, C.POINTER(C.c_double)]
    L.mpc_set_agent_fields.argtypes = [vp, vp, ci, vp, ci]
    L.mpc_fields_from_plans.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    L.mpc_closed_loop_traffic_field.argtypes = [vp, ci, ci, ci, ci, vp, vp, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mpc_default_roads.argtypes = [cp, C.POINTER(C.c_double)]
    L.mpc_set_agent_roads.argtypes = [vp, vp, ci, vp, ci]
    L.mpc_roads_from_script.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp]
    L.mpc_opponents_from_plans.argtypes = [vp, ci, ci, ci, vp, vp, C.c_double, vp, vp, vp]
    L.mpc_closed_loop_traffic.argtypes = [vp, ci, ci, ci, ci, vp, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mpc_obstacles_select.argtypes = [vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, C.c_double, vp, vp, vp]
    L.mpc_discs_from_obstacles.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp]
    L.mpc_fields_from_obstacles.argtypes = L.mpc_discs_from_obstacles.argtypes
    L.mpc_closed_loop_obstacles.argtypes = [vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                            vp, vp, vp, tp]
    L.mpc_rollout_held.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    L.mpc_obstacle_trigger.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, vp, C.c_double, vp, vp, C.c_double, ci, vp, vp, vp, vp, vp, vp]
    L.mpc_closed_loop_obstacles_event.argtypes = [vp, ci, ci, ci, C.POINTER(C.c_double), C.c_double, ci, ci, ci, ci, ci, ci, vp,
                                                  C.c_double, C.c_double, ci] + [vp] * 19 + [tp]
    L.mpc_opponent_trigger.argtypes = [vp, ci, ci, vp, vp, C.c_double, vp, vp, C.c_double, ci, vp, vp, vp, vp, vp, vp]
    L.mpc_closed_loop_traffic_event.argtypes = [vp, ci, ci, ci, C.POINTER(C.c_double), C.c_double, ci, ci, vp, vp, C.c_double,
                                                C.c_double, ci] + [vp] * 19
    L.mpc_step_lds_plan.argtypes = [ci, ci, ci, ci, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    L.mpc_math_probe.argtypes = [vp, ci, ci, vp, vp, vp, vp]
    L.mpc_lane_payoff.argtypes = [vp, ci, ci, C.POINTER(C.c_double), vp, vp, vp, vp, vp]
    L.mpc_set_profile.argtypes = [vp, ci]
    L.mpc_set_groups.argtypes = [vp, ci]
    L.mpc_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.mpc_last_kernel_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.mpc_set_solo_max.argtypes = [vp, ci]
    L.mpc_centerline_blocks.argtypes = [vp, vp, ci, vp]
    L.mpc_set_nearest_blocks.argtypes = [vp, ci]
    L.mpc_set_memo.argtypes = [vp, ci]
    L.mpc_set_round_limit.argtypes = [vp, C.c_int64]
    L.mpc_last_solo_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mpc_stream_concurrency.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mpc_set_poll_timeout.argtypes = [vp, C.c_double]
    L.mpc_debug_spin.argtypes = [vp, C.c_double, vp]
    L.mpc_debug_records.argtypes = [vp, ci, vp]
    L.mpc_debug_record_names.restype = C.c_char_p
    L.mpc_source_hash.restype = C.c_char_p
    for name in EXPORTS:
        if name not in ("mpc_last_error", "mpc_debug_record_names", "mpc_source_hash"):
            getattr(L, name).restype = ci
    _lib = L
    return L


def default_config(model=MODEL_PACEJKA, N=12, **overrides):
    """mpc_default_config + field overrides (arrays accept sequences)."""
    cfg = MpcConfig()
    rc = load().mpc_default_config(C.byref(cfg), int(model), int(N))
    if rc != 0:
        raise ValueError(load().mpc_last_error().decode())
    for k, v in overrides.items():
        cur = getattr(cfg, k)
        if hasattr(cur, "__len__"):
            for j, vv in enumerate(v):
                cur[j] = vv
        else:
            setattr(cfg, k, v)
    return cfg


def _default_row(fn, width, cfg):
    """The row of a per-agent table that `cfg` describes (library function `fn`), float64 [width]."""
    import numpy as np
    row = (C.c_double * width)()
    rc = getattr(load(), fn)(C.byref(cfg), row)
    if rc != 0:
        raise ValueError(load().mpc_last_error().decode())
    return np.array(row[:], dtype=np.float64)


def _default_table(who, default, cfg, P):
    """float64 [P, width] whose rows are default(cfg)"""
    import numpy as np
    if int(P) < 1:
        raise ValueError(f"{who}: P must be >= 1")
    return np.tile(default(cfg), (int(P), 1))


def _set_field(who, tab, name, val, off, widths):
    """Writes field `name` (columns from `off`) of the table from an every-row value -- a scalar where widths is (1,),
    else [w] -- or a per-row one -- [P], else [P, w] -- with w one of `widths`."""
    import numpy as np
    P = tab.shape[0]
    v = np.asarray(val, dtype=np.float64)
    if widths == (1,):
        if v.ndim == 0:
            v = np.full(P, float(v))
        if v.shape != (P,):
            raise ValueError(f"{who}: {name} must be a scalar or have shape ({P},), got {np.shape(val)}")
        tab[:, off] = v
        return
    if v.ndim == 1:
        v = np.tile(v, (P, 1))
    if v.ndim != 2 or v.shape[0] != P or v.shape[1] not in widths:
        shapes = [f"({w},)" for w in widths] + [f"({P}, {w})" for w in widths]
        raise ValueError(f"{who}: {name} must have shape {', '.join(shapes[:-1])} or {shapes[-1]}, got {np.shape(val)}")
    tab[:, off:off + v.shape[1]] = v


def default_params(cfg):
    """mpc_default_params: the row of the per-agent parameter table that `cfg` describes, float64 [NPARAM]."""
    return _default_row("mpc_default_params", NPARAM, cfg)


def param_rows(cfg, P, **overrides):
    """A parameter table for BatchedMPC.set_agent_params, on the host: float64 [P, NPARAM] whose rows are
    default_params(cfg) with overrides by field name -- `veh` [P, 22] (or [22]: every row), `cost_w` [P, 6] (or [6]),
    `accel`, `friction`, `v_ref` [P] (or a scalar).  Pure host code: usable without a GPU."""
    tab = _default_table("param_rows", default_params, cfg, P)
    for name, val in overrides.items():
        if name not in PARAM_FIELDS:
            raise ValueError(f"param_rows: unknown field {name!r} (one of {sorted(PARAM_FIELDS)})")
        off, width = PARAM_FIELDS[name]
        _set_field("param_rows", tab, name, val, off, (width,))
    return tab


def default_bounds(cfg):
    """mpc_default_bounds: the row of the per-agent bounds table that `cfg` describes, float64 [NBOUND]."""
    return _default_row("mpc_default_bounds", NBOUND, cfg)


def bound_rows(cfg, P, u_lb=None, u_ub=None):
    """A bounds table for BatchedMPC.set_agent_bounds, on the host: float64 [P, NBOUND] whose rows are
    default_bounds(cfg) with `u_lb` / `u_ub` [P, 2] (or [2]: every row) in their place.  Pure host code: usable
    without a GPU."""
    tab = _default_table("bound_rows", default_bounds, cfg, P)
    for name, val, off in (("u_lb", u_lb, 0), ("u_ub", u_ub, 2)):
        if val is not None:
            _set_field("bound_rows", tab, name, val, off, (2,))
    return tab


def default_constraints(cfg):
    """mpc_default_constraints: the row of the per-agent constraint table that `cfg` describes, float64 [NCONSTR]."""
    return _default_row("mpc_default_constraints", NCONSTR, cfg)


def constraint_rows(cfg, P, g_off=None, D_lb=None, D_ub=None, lane_halfwidth=None):
    """A constraint table for BatchedMPC.set_agent_constraints, on the host: float64 [P, NCONSTR] whose rows are
    default_constraints(cfg) with `g_off` / `D_lb` / `D_ub` [P, k] (or [k]: every row; k = nx or 6 leading entries) and
    `lane_halfwidth` [P] (or a scalar) in their place.  Pure host code: usable without a GPU."""
    tab = _default_table("constraint_rows", default_constraints, cfg, P)
    nx = 6 if cfg.model == MODEL_PACEJKA else 4
    for name, val, widths in (("g_off", g_off, (nx, 6)), ("D_lb", D_lb, (nx, 6)), ("D_ub", D_ub, (nx, 6)),
                              ("lane_halfwidth", lane_halfwidth, (1,))):
        if val is not None:
            _set_field("constraint_rows", tab, name, val, CONSTR_FIELDS[name][0], widths)
    return tab


def disc_row_width(cfg):
    """MPC_DISC_ROW(N): doubles per row of the disc table of `cfg`'s horizon."""
    return 3 * NDISC * int(cfg.N)


def default_discs(cfg):
    """mpc_default_discs: the row of the disc table that says "no obstacle at any stage", float64 [3 NDISC N] of zeros."""
    return _default_row("mpc_default_discs", disc_row_width(cfg), cfg)


def disc_rows(cfg, P, centres=None, radii=None):
    """A disc table for BatchedMPC.set_agent_discs, on the host: float64 [P, 3 NDISC N], row layout [N][NDISC][3] =
    (cx, cy, r), default_discs(cfg) with `centres` [P, N, NDISC, 2] (or [N, NDISC, 2]: every row) and `radii`
    [P, N, NDISC] (or [N, NDISC]: every row; or a scalar) in their place.  Pure host code: usable without a GPU."""
    import numpy as np
    tab = _default_table("disc_rows", default_discs, cfg, P)
    P, N = tab.shape[0], int(cfg.N)
    v = tab.reshape(P, N, NDISC, 3)          # a view: writes land in tab
    if centres is not None:
        c = np.asarray(centres, dtype=np.float64)
        if c.shape not in ((N, NDISC, 2), (P, N, NDISC, 2)):
            raise ValueError(f"disc_rows: centres must have shape ({N}, {NDISC}, 2) or ({P}, {N}, {NDISC}, 2), got {c.shape}")
        v[..., :2] = c
    if radii is not None:
        r = np.asarray(radii, dtype=np.float64)
        if r.shape not in ((), (N, NDISC), (P, N, NDISC)):
            raise ValueError(f"disc_rows: radii must be a scalar or have shape ({N}, {NDISC}) or ({P}, {N}, {NDISC}), got {r.shape}")
        v[..., 2] = r
    return tab


def default_rates(cfg):
    """mpc_default_rates: the row of the rate table that says "no move penalty", float64 [NRATE] of zeros."""
    return _default_row("mpc_default_rates", NRATE, cfg)


def rate_rows(w_d, w_delta, u_prev=None):
    """A rate table for BatchedMPC.set_agent_rates, on the host: float64 [P, NRATE], rows [w_d, w_delta, d_prev,
    delta_prev].  w_d and w_delta: scalars or [P] (a scalar beside a [P] is every row's), finite and >= 0; u_prev: the
    input applied last, [2] (every row) or [P, 2], finite; None: zeros.  P is the longest of the three (1 when all are
    scalars / [2]).  Pure host code: usable without a GPU."""
    import numpy as np
    wd, wl = np.asarray(w_d, dtype=np.float64), np.asarray(w_delta, dtype=np.float64)
    up = np.zeros(2) if u_prev is None else np.asarray(u_prev, dtype=np.float64)
    if wd.ndim > 1 or wl.ndim > 1:
        raise ValueError(f"rate_rows: w_d and w_delta must be scalars or have shape (P,), got {wd.shape} and {wl.shape}")
    if up.ndim not in (1, 2) or up.shape[-1] != 2:
        raise ValueError(f"rate_rows: u_prev must have shape (2,) or (P, 2), got {up.shape}")
    sizes = {int(a.shape[0]) for a, nd in ((wd, 1), (wl, 1), (up, 2)) if a.ndim == nd}
    if len(sizes) > 1 or 0 in sizes:
        raise ValueError(f"rate_rows: w_d, w_delta and u_prev disagree about the number of rows P >= 1: {sorted(sizes)}")
    P = sizes.pop() if sizes else 1
    for name, a in (("w_d", wd), ("w_delta", wl)):
        if not np.all(np.isfinite(a)) or np.any(a < 0.0):
            raise ValueError(f"rate_rows: {name} must be finite and >= 0")
    if not np.all(np.isfinite(up)):
        raise ValueError("rate_rows: u_prev must be finite")
    tab = np.empty((P, NRATE), dtype=np.float64)
    tab[:, 0], tab[:, 1], tab[:, 2:] = wd, wl, up
    return tab


def field_row(N):
    """MPC_FIELD_ROW(N): doubles per row of the field table of a horizon of N stages."""
    return NFIELD * NFSRC * int(N)


def default_fields(cfg):
    """mpc_default_fields: the row of the field table that says "no obstacle at any stage", float64 [field_row(N)] of
    zeros."""
    return _default_row("mpc_default_fields", field_row(cfg.N), cfg)


def field_rows(centres, heading, A, sigma_x, sigma_y, alpha=0):
    """A field table for BatchedMPC.set_agent_fields, on the host: float64 [P, N, NFIELD, NFSRC], sources
    [cx, cy, cos heading, sin heading, A, 1 / (2 sigma_x^2), 1 / (2 sigma_y^2), alpha] (reshape(P, -1) is the table).
    centres: [P, N, NFIELD, 2], or anything that broadcasts to it ([2]: the same standing point in every slot of every
    stage).  heading, A, sigma_x, sigma_y, alpha: scalars or arrays that broadcast to [P, N, NFIELD]; A >= 0 (0: the
    slot holds no source -- A = [0.3, 0] fills slot 0 alone), sigma > 0, everything finite.  Pure host code: usable
    without a GPU."""
    import numpy as np
    c = np.asarray(centres, dtype=np.float64)
    if c.ndim < 1 or c.shape[-1] != 2:
        raise ValueError(f"field_rows: centres must end in a dimension of 2 (x, y), got {c.shape}")
    if c.ndim > 4 or (c.ndim >= 2 and c.shape[-2] not in (1, NFIELD)):
        raise ValueError(f"field_rows: centres must broadcast to (P, N, {NFIELD}, 2), got {c.shape}")
    c = c.reshape((1,) * (4 - c.ndim) + c.shape)
    others = [np.asarray(v, dtype=np.float64) for v in (heading, A, sigma_x, sigma_y, alpha)]
    if any(v.ndim > 3 for v in others):
        raise ValueError(f"field_rows: heading, A, sigma_x, sigma_y and alpha must broadcast to (P, N, {NFIELD})")
    try:
        shape = np.broadcast_shapes(c.shape[:3], (1, 1, NFIELD), *(v.shape for v in others))
    except ValueError:
        raise ValueError("field_rows: the arguments do not broadcast to one (P, N, NFIELD)") from None
    if shape[2] != NFIELD:
        raise ValueError(f"field_rows: {NFIELD} sources per stage, got {shape[2]}")
    hd, Av, sx, sy, al = (np.broadcast_to(v, shape) for v in others)
    for name, v in (("centres", c), ("heading", hd), ("A", Av), ("sigma_x", sx), ("sigma_y", sy), ("alpha", al)):
        if not np.all(np.isfinite(v)):
            raise ValueError(f"field_rows: {name} must be finite")
    if np.any(Av < 0.0):
        raise ValueError("field_rows: A must be >= 0")
    if np.any(sx <= 0.0) or np.any(sy <= 0.0):
        raise ValueError("field_rows: sigma_x and sigma_y must be > 0")
    tab = np.empty(shape + (NFSRC,), dtype=np.float64)
    tab[..., 0:2] = np.broadcast_to(c, shape + (2,))
    tab[..., 2], tab[..., 3], tab[..., 4] = np.cos(hd), np.sin(hd), Av
    tab[..., 5], tab[..., 6], tab[..., 7] = 1.0 / (2.0 * sx * sx), 1.0 / (2.0 * sy * sy), al
    return tab


def obstacle_width(cfg):
    """W of a sample of the obstacle tracks of `cfg`: 3 = (cx, cy, r) on CONSTR_DISCS, NFSRC (a whole risk source) else."""
    return 3 if int(cfg.constr_mode) == CONSTR_DISCS else NFSRC


def obstacle_tracks(cfg, centres=None, radii=None, sources=None):
    """The table of scripted obstacles for BatchedMPC.obstacles_select / closed_loop_obstacles, on the host: float64
    [scenes, K, Lt, W], one sample per Ts.  On a cfg of CONSTR_DISCS (W = 3): `centres` [scenes, K, Lt, 2] and `radii`
    [scenes, K, Lt] (or anything that broadcasts to it; r = 0: the obstacle is absent at that sample).  On every other cfg
    (W = NFSRC): `sources` [scenes, K, Lt, NFSRC] = [cx, cy, c, s, A, kx, ky, alpha] (A = 0: absent).  Checked by the row
    rules of mpc_set_agent_discs / mpc_set_agent_fields -- the library does not check the table: everything finite,
    r >= 0; A, kx, ky >= 0 and a skew (alpha != 0) only with kx > 0; 1 <= K <= SCENE_MAX, Lt >= 1.  Pure host code."""
    import numpy as np
    who = "obstacle_tracks"
    if obstacle_width(cfg) == 3:
        if centres is None or radii is None or sources is not None:
            raise ValueError(f"{who}: a configuration of CONSTR_DISCS takes centres and radii (an obstacle is a disc)")
        c = np.asarray(centres, dtype=np.float64)
        if c.ndim != 4 or c.shape[-1] != 2:
            raise ValueError(f"{who}: centres must have shape (scenes, K, Lt, 2), got {c.shape}")
        try:
            r = np.broadcast_to(np.asarray(radii, dtype=np.float64), c.shape[:3])
        except ValueError:
            raise ValueError(f"{who}: radii must broadcast to {c.shape[:3]}, got {np.shape(radii)}") from None
        tab = np.empty(c.shape[:3] + (3,), dtype=np.float64)
        tab[..., :2], tab[..., 2] = c, r
        if not np.all(np.isfinite(tab)):
            raise ValueError(f"{who}: (cx, cy, r) must be finite")
        if np.any(tab[..., 2] < 0.0):
            raise ValueError(f"{who}: the radius must not be negative")
    else:
        if sources is None or centres is not None or radii is not None:
            raise ValueError(f"{who}: a configuration without CONSTR_DISCS takes sources (an obstacle is a risk source)")
        tab = np.array(sources, dtype=np.float64)
        if tab.ndim != 4 or tab.shape[-1] != NFSRC:
            raise ValueError(f"{who}: sources must have shape (scenes, K, Lt, {NFSRC}), got {tab.shape}")
        if not np.all(np.isfinite(tab)):
            raise ValueError(f"{who}: (cx, cy, c, s, A, kx, ky, alpha) must be finite")
        if np.any(tab[..., 4:7] < 0.0):
            raise ValueError(f"{who}: A, kx and ky must not be negative")
        if np.any((tab[..., 7] != 0.0) & ~(tab[..., 5] > 0.0)):
            raise ValueError(f"{who}: a skew (alpha != 0) needs kx > 0")
    if tab.shape[0] < 1 or not 1 <= tab.shape[1] <= SCENE_MAX or tab.shape[2] < 1:
        raise ValueError(f"{who}: need scenes >= 1, 1 <= K <= {SCENE_MAX} obstacles and Lt >= 1 samples, got {tab.shape[:3]}")
    return np.ascontiguousarray(tab)


def default_roads(cfg):
    """mpc_default_roads: the row of the road table in which no part is on at any stage, float64 [NROAD * N] of zeros."""
    return _default_row("mpc_default_roads", NROAD * int(cfg.N), cfg)


def road_rows(N, offset=0.0, w_offset=0.0, lo=0.0, w_lo=0.0, hi=0.0, w_hi=0.0, v_target=0.0, w_speed=0.0):
    """A road table for BatchedMPC.set_agent_roads, on the host: float64 [P, N, NROAD], stage entries
    [offset, w_offset, lo, w_lo, hi, w_hi, v_target, w_speed] (reshape(P, -1) is the table).  Every argument is a scalar
    or an array that broadcasts to [P, N] ([N]: the same profile for every row; [P, 1]: one value per row).  offset, lo
    and hi are values of the signed lateral offset e from the centerline, POSITIVE TO THE RIGHT of the direction of
    travel; a weight of 0 switches its part off.  Everything finite, weights >= 0, lo <= hi wherever both edge weights
    are non-zero.  Pure host code: usable without a GPU."""
    import numpy as np
    N = int(N)
    if N < 1:
        raise ValueError("road_rows: N must be >= 1")
    names = ("offset", "w_offset", "lo", "w_lo", "hi", "w_hi", "v_target", "w_speed")
    vals = [np.asarray(v, dtype=np.float64) for v in (offset, w_offset, lo, w_lo, hi, w_hi, v_target, w_speed)]
    if any(v.ndim > 2 for v in vals):
        raise ValueError("road_rows: the arguments must broadcast to (P, N)")
    try:
        shape = np.broadcast_shapes((1, N), *(v.shape for v in vals))
    except ValueError:
        raise ValueError("road_rows: the arguments do not broadcast to one (P, N)") from None
    if shape[1] != N:
        raise ValueError(f"road_rows: {N} stages per row, got {shape[1]}")
    tab = np.empty(shape + (NROAD,), dtype=np.float64)
    for i, (name, v) in enumerate(zip(names, vals)):
        if not np.all(np.isfinite(v)):
            raise ValueError(f"road_rows: {name} must be finite")
        if name.startswith("w_") and np.any(v < 0.0):
            raise ValueError(f"road_rows: {name} must be >= 0")
        tab[..., i] = np.broadcast_to(v, shape)
    if np.any((tab[..., 3] != 0.0) & (tab[..., 5] != 0.0) & (tab[..., 2] > tab[..., 4])):
        raise ValueError("road_rows: lo must not exceed hi where both edge weights are non-zero")
    return tab


def track_init(cfg, K, L, stride, lead, closed):
    """mpc_track_init: the geometry (an MpcTrack, R filled in) of the window table of K tracks of L points each for
    `cfg`'s S, or ValueError with the library's reason.  Pure host code: usable without a GPU."""
    t = MpcTrack()
    rc = load().mpc_track_init(C.byref(t), C.byref(cfg), int(K), int(L), int(stride), int(lead), int(bool(closed)))
    if rc != 0:
        raise ValueError(load().mpc_last_error().decode())
    return t


def library_hash():
    """The source hash the RUNNING library was built from (mpc_source_hash)."""
    return load().mpc_source_hash().decode()


class MpcError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        raise MpcError(f"libmpc_hip error {rc}: {load().mpc_last_error().decode()}")
