/*
 * mpc_hip.h -- C-ABI of libmpc_hip.so, the MI355X (gfx950) batched MPC solve step.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference
 * (pure Python) reaches its solver through pybind11/dlopen:
 *     controller.py:27-49   pa.ALMSolver(alm_params, inner_solver=pa.StructuredPANOCLBFGSSolver(..))
 *     controller.py:57      x, y, stats = solver(problem, x, y)
 *     main.py:54-56         generate_and_compile_casadi_problem(f, g); prob.C.lowerbound/upperbound
 *     car_dynamics.py:159   f_d.mapaccum(N)(y0, u, p)          (rollout / plant step)
 * A maintainer binds the entry points below with ctypes.
 *
 * Conventions
 *  - plain pointers and sizes only; every data pointer is a DEVICE pointer (HBM) owned by
 *    the caller; the library owns only its handle and its scratch workspace.
 *  - batch arrays are agent-major row-major: x0 [B][nx], U [B][2N] with the reference's
 *    flat stage-major order [d0, delta0, d1, delta1, ...] (car_dynamics.py:149-157),
 *    lambda [B][m], stats [B][MPC_NSTATS].
 *  - centerlines: table cl [C][2S], each row flat [x_0..x_{S-1}, y_0..y_{S-1}]
 *    (main.py:113 ravel(order='F')); cl_index [B] int32 selects a row per agent, NULL = row 0.
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*) except
 *    mpc_solve_batch / mpc_solve_active / mpc_closed_loop / mpc_closed_loop_event / mpc_closed_loop_track, which poll
 *    device counters and return when the batch is solved.
 *  - between mpc_solve_batch_async and mpc_solve_wait the handle belongs to its worker thread: every
 *    other call on it returns MPC_E_ARG without touching it.
 *  - return value: 0 on success, negative MPC_E_* otherwise; mpc_last_error() explains.
 *    No exceptions cross the ABI.  One handle per GPU/stream; a handle is not thread-safe.
 */
#ifndef MPC_HIP_H
#define MPC_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { MPC_MODEL_KINEMATIC = 0, /* dynamics.py:122-173, nx = 4 [x, y, phi, v] */
       MPC_MODEL_PACEJKA = 1 }; /* car_dynamics.py:93-129, nx = 6 [x, y, phi, vx, vy, omega] */
enum { MPC_WRAP_FLOOR = 0, MPC_WRAP_FMOD = 1, MPC_WRAP_IEEE = 2 }; /* car_dynamics.py:168-172 */
enum { MPC_CONSTR_NONE = 0,     /* m = 0 (== main.py:57 left commented: D = R^m) */
       MPC_CONSTR_STATE_SQ = 1, /* main.py:43-52: g = x_i^2 - off_i per stage, bounds D_lb/D_ub */
       MPC_CONSTR_LANE = 2,     /* signed lateral distance to the centerline within +-halfwidth */
       MPC_CONSTR_DISCS = 3 };  /* MPC_NDISC keep-out discs per stage and agent (mpc_set_agent_discs): m = MPC_NDISC N */
/* alpaqa SolverStatus values read at controller.py:59-64 */
enum { MPC_ST_UNKNOWN = 0, MPC_ST_CONVERGED = 1, MPC_ST_MAXTIME = 2, MPC_ST_MAXITER = 3,
       MPC_ST_NOTFINITE = 4, MPC_ST_NOPROGRESS = 5, MPC_ST_INTERRUPTED = 6 };
enum { MPC_OK = 0, MPC_E_ARG = -1, MPC_E_HIP = -2, MPC_E_ALLOC = -3, MPC_E_LIMIT = -4 };

#define MPC_NSTATS 8 /* [status, outer_iters, inner_iters, inner_failures, eps, delta, psi, n_evals] */
#define MPC_MAX_N 64 /* horizon limit */
#define MPC_NREC 64  /* doubles per agent of mpc_debug_records */

typedef struct mpc_config {
    int32_t model;           /* MPC_MODEL_* */
    int32_t N;               /* horizon (main.py:68) */
    int32_t S;               /* centerline points (main.py:70) */
    int32_t nfe;             /* RK4 finite elements per stage (car_dynamics.py:136) */
    int32_t wrap_mode;       /* MPC_WRAP_* */
    int32_t clip_inputs;     /* dynamics.py:99,:163 np.clip of the inputs inside the RHS */
    int32_t constr_mode;     /* MPC_CONSTR_* */
    int32_t lbfgs_memory;    /* controller.py:36 */
    int32_t max_iter;        /* controller.py:31 */
    int32_t max_outer;       /* controller.py:45 */
    int32_t hess_heuristic;  /* controller.py:32 */
    int32_t max_no_progress; /* alpaqa default 10 */
    double Ts;               /* car_dynamics.py:93 */
    double v_ref;            /* main.py:65 */
    double cost_w[6];        /* car_dynamics.py:230 */
    double veh[22];          /* car_dynamics.py:65-88 order; main.py:82-111 values */
    double accel, friction;  /* dynamics.py:34-35 */
    double u_lb[2], u_ub[2]; /* main.py:55-56, order [d, delta] */
    double g_off[6];         /* main.py:46-51 */
    double D_lb[6], D_ub[6]; /* main.py:57 */
    double lane_halfwidth;
    double alm_eps, alm_delta, Sigma0, eps0, rho, Delta, theta, M, Sigma_max; /* controller.py:40-43 */
    double Delta_lower, Sigma0_lower, eps0_increase, rho_increase;
    int32_t max_num_initial_retries, max_num_retries, max_total_num_retries;
    int32_t max_total_inner; /* iteration budget replacing controller.py:30,:44 wall-clock caps */
    int32_t max_total_evals; /* evaluation budget (0 = none), checked in the inner stop test where
                                alpaqa checks the clock: status MaxTime (2) when hit */
    double lip_eps, lip_delta, Lgamma_factor, L_min, L_max, tau_min, qub_tol;
} mpc_config;

typedef struct mpc_handle mpc_handle;

/* fills *cfg with the reference's constants (main.py:65-111, controller.py:27-48) */
int mpc_default_config(mpc_config *cfg, int model, int N);
int mpc_nx(const mpc_config *cfg);
int mpc_m(const mpc_config *cfg);

/* replaces controller.py:12-49 (solver construction) + main.py:25-59 (problem construction) */
int mpc_create(const mpc_config *cfg, int device, mpc_handle **out);
int mpc_destroy(mpc_handle *h);
const char *mpc_last_error(void);
/* identity of the build: SHA-256 over the library's sources and this header as _lib.build() compiled them
 * ("unknown" for a build by other means).  Committed profiles name the build they measured by it and bench.py
 * uses a profile's counters only when it matches the running library. */
const char *mpc_source_hash(void);
/* host-only: how the round path's step kernel with the L-BFGS history in LDS is launched for an n-variable problem
 * with memory M and m constraints -- the history pairs P it copies into LDS (lds_pairs > 0: the MPC_LDS_PAIRS
 * override), the launch's dynamic LDS bytes per workgroup (chain != 0: with the thread-per-agent chain blocks) and
 * the waves per SIMD (= workgroups per CU) the kernel is compiled for, which P is sized to let share a CU */
int mpc_step_lds_plan(int n, int M, int m, int chain, int lds_pairs, int *pairs, int *lds_bytes, int *waves_per_simd);

/* Per-agent vehicle and cost parameters: a table of P rows in device memory and one row index per agent, beside
 * the centerline table.  One row, all doubles: [0..21] veh (car_dynamics.py:65-88 order, as mpc_config.veh),
 * [22] accel, [23] friction (dynamics.py:34-35), [24] v_ref, [25..30] cost_w (car_dynamics.py:230) -- in the
 * reference these are run-time data of the problem (main.py:30, :119 `prob.param`), not part of its construction.
 * mpc_default_params (host only): the row `cfg` describes.
 * mpc_set_agent_params: table == NULL unbinds (the handle is then what it was before).  Bound, the calls that
 * evaluate the model -- mpc_rhs, mpc_rollout, mpc_stage_cost, mpc_eval_cost_grad(_wave), mpc_solve_batch(_async),
 * mpc_solve_active, mpc_closed_loop(_event) -- use row index[b] for agent b and return MPC_E_ARG for a batch size other than B;
 * mpc_closed_loop(_event) advance the plant with row plant_index[b] (NULL: the same rows; main.py:145's separate `param`).
 * The input box, the constraint data, Ts, N and every solver parameter stay the handle's.  table [P][MPC_NPARAM],
 * index [B] and plant_index [B] are DEVICE memory of the caller, read at every call: rows may be rewritten in place
 * between calls without binding again.  The P rows are checked once, at bind time, through a synchronous copy:
 * every value finite, veh[1] + veh[2] > 0, and on the Pacejka model veh[7] > 0 and veh[8] > 0; index ranges are the
 * caller's to check (the Python front end does).  Refused (MPC_E_ARG) while an asynchronous solve is in flight. */
#define MPC_NPARAM 31
int mpc_default_params(const mpc_config *cfg, double *row);
int mpc_set_agent_params(mpc_handle *h, const double *table, int P, const int32_t *index,
                         const int32_t *plant_index, int B);

/* Per-agent input bounds: a table of P boxes in device memory and one row index per agent, beside the parameter table.
 * One row, all doubles: [u_lb[0], u_lb[1], u_ub[0], u_ub[1]] = [d_min, delta_min, d_max, delta_max] -- in the reference
 * the box C is run-time data of the problem (main.py:55-56 `prob.C.lowerbound / upperbound`), not part of its
 * construction.
 * mpc_default_bounds (host only): the row `cfg` describes.
 * mpc_set_agent_bounds: table == NULL unbinds (the handle is then what it was before).  Bound, the calls that project
 * onto the box -- mpc_prox_step, mpc_solve_batch(_async), mpc_solve_active, mpc_closed_loop(_event) -- use row index[b]
 * for agent b and return MPC_E_ARG for a batch size other than B; no other entry point reads the box (clip_inputs
 * clips to veh's max_drive / max_steer, which the parameter row carries).  Ts, N, the constraint data and every solver
 * parameter stay the handle's.  The table is independent of the parameter table: either, both or neither may be bound;
 * bound together they are for the same B (MPC_E_ARG otherwise), each with its own index.  table [P][MPC_NBOUND] and
 * index [B] are DEVICE memory of the caller, read at every call: rows may be rewritten in place between calls without
 * binding again.  The P rows are checked once, at bind time, through a synchronous copy, by the rule mpc_create applies
 * to the handle's box: u_lb[i] <= u_ub[i] (a NaN fails it, infinities pass); index ranges are the caller's to check
 * (the Python front end does).  Refused (MPC_E_ARG) while an asynchronous solve is in flight.  A table whose rows equal
 * the handle's box gives the bits of the solve without a table. */
#define MPC_NBOUND 4
int mpc_default_bounds(const mpc_config *cfg, double *row);
int mpc_set_agent_bounds(mpc_handle *h, const double *table, int P, const int32_t *index, int B);

/* Per-agent constraint data: a table of P rows in device memory and one row index per agent, beside the two tables above.
 * One row, all doubles: [0..5] g_off, [6..11] D_lb, [12..17] D_ub, [18] lane_halfwidth -- the data of the general
 * constraints (main.py:43-52 `g_i = x_i^2 - g_off[i]` within `[D_lb[i], D_ub[i]]`; the lane band `|signed distance| <=
 * lane_halfwidth`).  Only the fields of the handle's constr_mode are read: MPC_CONSTR_STATE_SQ reads the first nx entries
 * of the three vectors, MPC_CONSTR_LANE reads [18].
 * mpc_default_constraints (host only): the row `cfg` describes.
 * mpc_set_agent_constraints: table == NULL unbinds (the handle is then what it was before).  Bound, the calls that read
 * constraint data -- mpc_eval_cost_grad, mpc_eval_cost_grad_wave, mpc_solve_batch(_async), mpc_solve_active,
 * mpc_closed_loop(_event) -- use row index[b] for agent b and return MPC_E_ARG for a batch size other than B; no other
 * entry point reads constraint data.  constr_mode, m, N, Ts, the input box and every ALM and PANOC parameter (Sigma0,
 * alm_delta, M, ...) stay the handle's.  The table is independent of the other two: any subset of the three may be
 * bound; bound together they are for the same B (MPC_E_ARG otherwise), each with its own index.  table [P][MPC_NCONSTR]
 * and index [B] are DEVICE memory of the caller, read at every call: rows may be rewritten in place between calls
 * without binding again.  The P rows are checked once, at bind time, through a synchronous copy: D_lb[i] <= D_ub[i] for
 * i < nx (a NaN fails it, infinities pass) and g_off finite (MPC_CONSTR_STATE_SQ); lane_halfwidth finite and > 0
 * (MPC_CONSTR_LANE); mpc_create itself checks neither.  Index ranges are the caller's to check (the Python front end
 * does).  Refused (MPC_E_ARG) while an asynchronous solve is in flight, and on a handle with MPC_CONSTR_NONE: there is
 * nothing to bind to.  A table whose rows equal the handle's values gives the bits of the call without a table. */
#define MPC_NCONSTR 19
int mpc_default_constraints(const mpc_config *cfg, double *row);
int mpc_set_agent_constraints(mpc_handle *h, const double *table, int P, const int32_t *index, int B);

/* Per-agent, per-stage keep-out discs (constr_mode MPC_CONSTR_DISCS): a table of P rows in device memory and one row
 * index per agent, beside the three tables above -- the one table whose data varies with the stage.  One row, all
 * doubles: [N][MPC_NDISC][3] = (cx, cy, r), MPC_DISC_ROW(N) of them.  Constraint kk = MPC_NDISC k + j of an agent is disc
 * j of stage k, taken -- as every general constraint is -- at the state at the end of stage k (x_{k+1}):
 *     dx = x - cx, dy = y - cy, g = (dx dx + dy dy) - r r   within [0, +inf)
 * every operation rounded on its own.  A disc with r = 0 is vacuous (g = d^2 >= 0): that is how "no obstacle at this
 * stage" is said.  The bounds [0, +inf) are the same for every agent; g_off, D_lb, D_ub and lane_halfwidth of the
 * configuration are not read in this mode.
 * mpc_default_discs (host only): a row of zeros, MPC_DISC_ROW(cfg->N) doubles.
 * mpc_set_agent_discs: table == NULL unbinds.  The discs have no shared value to fall back on: on a handle of
 * MPC_CONSTR_DISCS the calls that evaluate constraints -- mpc_eval_cost_grad(_wave), mpc_solve_batch(_async),
 * mpc_solve_active, mpc_closed_loop(_event, _track) -- return MPC_E_ARG before any launch while no disc table is bound;
 * bound, they use row index[b] for agent b and return MPC_E_ARG for a batch size other than B.  The table is independent
 * of the parameter and bounds tables: any of them may be bound beside it; bound together they are for the same B
 * (MPC_E_ARG otherwise), each with its own index.  table [P][MPC_DISC_ROW(N)] and index [B] are DEVICE memory of the
 * caller, read at every call: rows may be rewritten in place between calls without binding again (a host loop of solves
 * that moves the obstacles does exactly that).  The P rows are checked once, at bind time, through a synchronous copy:
 * every value finite and r >= 0; index ranges are the caller's to check (the Python front end does).  Refused
 * (MPC_E_ARG) while an asynchronous solve is in flight and on a handle of another constr_mode;
 * mpc_set_agent_constraints is refused on a handle of MPC_CONSTR_DISCS (there is no constraint data to bind).
 * The closed loops read the table as it is bound -- obstacles standing on the track: stage k of every re-plan reads
 * entry k of the agent's row.
 * mpc_discs_from_plans: the gather for inter-agent avoidance, asynchronous on `stream`.  X [B][N][nx] is what
 * mpc_rollout wrote for the agents' current plans, opp [B][MPC_NDISC] (int32) the opponents of agent b (< 0 or >= B:
 * none), radius [B] the radius of agent b as an obstacle; table [B][MPC_DISC_ROW(N)] receives
 * table[b][k][j] = (X[o][k][0], X[o][k][1], radius[o]) for o = opp[b][j], or zeros where there is no opponent.  Every
 * word written is a copy of an input word or zero.  With index = 0 .. B-1 bound this is "everyone avoids everyone's
 * last plan", one sweep of an iterated best response, without leaving the device.  All four are device memory. */
#define MPC_NDISC 2
#define MPC_DISC_ROW(N) (3 * MPC_NDISC * (N))
int mpc_default_discs(const mpc_config *cfg, double *row);
int mpc_set_agent_discs(mpc_handle *h, const double *table, int P, const int32_t *index, int B);
int mpc_discs_from_plans(mpc_handle *h, int B, const double *X, const int32_t *opp, const double *radius, double *table,
                         void *stream);

/* Traffic: who the opponents are, decided on the device, and the closed loop around it.
 * Scenes are contiguous blocks of G agents: agent b belongs to scene b / G, 1 <= G <= MPC_SCENE_MAX and B % G == 0
 * (unequal scenes are the caller's to pad); agents of different scenes never see each other.
 * mpc_opponents_from_plans: X [B][Nst][nx] are positions per stage as mpc_rollout writes them (Nst = 1 with X = x:
 * the states as they are now), radius [B] the radius of agent b as an obstacle; opp [B][MPC_NDISC] (int32, out) and
 * clear [B][MPC_NDISC] (out, NULL ok).  All four are DEVICE memory; asynchronous on `stream`.  The rule, every operation
 * rounded on its own (a host loop in IEEE doubles gets the same bits): for o != b of b's scene and stage k < Nst
 *     dx = X[b][k][0] - X[o][k][0], dy = X[b][k][1] - X[o][k][1], g_k = (dx dx + dy dy) - r_o r_o,   c(b, o) = min_k g_k
 * -- the disc expression above, operand for operand, so c is the smallest constraint value the next solve sees at the
 * current plans.  A pair with a g_k that is not finite is no candidate (a diverged agent does not poison its scene);
 * o is a candidate iff c(b, o) < reach reach (reach >= 0; +inf: all).  Selected are the MPC_NDISC candidates smallest
 * in the lexicographic order (c, o): slot 0 holds the smallest, ties go to the smaller agent index; opp holds GLOBAL
 * agent indices, an unused slot opp = -1 and clear = +inf.  No atomics: the same input gives the same output.  Works
 * on a handle of any constr_mode (it reads nx alone); radius is device data and is not checked.  MPC_E_ARG, before any
 * launch: G outside [1, MPC_SCENE_MAX], B % G != 0, Nst < 1, reach negative or NaN, NULL X, radius or opp, an
 * asynchronous solve in flight, and, with tables bound, a B other than the bound one.
 * mpc_closed_loop_traffic: T closed-loop steps in which every agent avoids the current plans of the nearest agents of
 * its scene.  Blocking; the arguments it shares with mpc_closed_loop mean what they mean there (the plant's parameter
 * rows and `shift` included).  Only on a handle of MPC_CONSTR_DISCS; `table` must be the disc table currently bound, with
 * P == B rows (MPC_E_ARG otherwise) -- the loop rewrites it in place; its index being 0 .. B-1 is the caller's to ensure
 * (the Python front end does).  Step t, every numbered launch being the one the public call of that name makes:
 *   1. X = mpc_rollout(x, U), N stages, into a buffer of the handle
 *   2. opp = the selection above on X (G, radius, reach); traj_opp [B][T][MPC_NDISC] records it (NULL ok)
 *   3. table = mpc_discs_from_plans(X, opp, radius)
 *   4. mpc_solve_batch; U and lambda are warm starts as the step before left them.  lambda is NOT re-slotted when an
 *      agent's opponents change: a multiplier that belonged to another opponent is a warm start like any other, and the
 *      augmented Lagrangian absorbs it
 *   5. the plant step of mpc_closed_loop: u0, the plant's rows, shift, traj_x, traj_u, fail_count
 *   6. traj_clear [B][T] (NULL ok) = slot 0 of `clear` of the selection on the NEW states (Nst = 1, reach = +inf): the
 *      realised worst clearance of agent b at time t + 1, d^2 - r_o^2 to the nearest agent of its scene; +inf for G = 1
 * Nothing but the solve's own polls returns to the host. */
#define MPC_SCENE_MAX 64
int mpc_opponents_from_plans(mpc_handle *h, int B, int G, int Nst, const double *X, const double *radius, double reach,
                             int32_t *opp, double *clear, void *stream);
int mpc_closed_loop_traffic(mpc_handle *h, int B, int T, int shift, int G, const double *radius, double reach,
                            double *x, const double *cl, const int32_t *cl_index, double *U, double *lambda,
                            double *table, double *traj_x, double *traj_u, int32_t *traj_opp, double *traj_clear,
                            int32_t *fail_count, double *stats, void *stream);

/* Input-rate cost: per-agent move penalties and the input applied last -- a fifth table of P rows in device memory and one
 * row index per agent.  One row, MPC_NRATE doubles: [w_d, w_delta, d_prev, delta_prev].  With u_k = (d_k, delta_k) the
 * decision variables of stage k (as they are, before the model clips them) and u_{-1} = (d_prev, delta_prev), stage k's
 * cost -- behind the six terms of the reference and before the ALM terms -- gets the move penalty, and the stage's direct
 * input gradient its derivative, every operation rounded on its own and in this order (i = 0 drive, 1 steering):
 *     e_i = u_k[i] - u_{k-1}[i],   t_i = w_i e_i,   L_k = L_k + (t_0 e_0 + t_1 e_1)
 *     dL/du_k[i] = dL/du_k[i] + 2 t_i;   and for k < N - 1:   f_i = u_{k+1}[i] - u_k[i],   dL/du_k[i] = dL/du_k[i] - 2 (w_i f_i)
 * psi stays the sum of the stage costs in stage order.  The four evaluation routes (K1b, the fused K1b + K1c kernel, the
 * wave evaluation, the persistent kernel) call one device function, so a request gets the same bits whichever serves
 * it.  Zero weights change no bit of a solve.  The table is read by mpc_eval_cost_grad(_wave), mpc_solve_batch(_async),
 * mpc_solve_active and the closed loops; mpc_stage_cost, mpc_rhs, mpc_rollout and mpc_prox_step do not read it (a single
 * stage has no neighbour).  Handles of every constr_mode take it (MPC_CONSTR_DISCS: beside the disc table).
 * mpc_default_rates (host only): a row of zeros.
 * mpc_set_agent_rates: the semantics of the other tables.  table == NULL unbinds; bound, the calls above use row
 * index[b] for agent b and return MPC_E_ARG for a batch size other than B; bound beside other tables it is for the same
 * B.  table [P][MPC_NRATE] and index [B] are DEVICE memory of the caller, read at every call: rows may be rewritten in
 * place between calls (a host loop writes the input it applies into columns 2 and 3).  The P rows are checked once, at
 * bind time: all four values finite, both weights >= 0.  Refused (MPC_E_ARG) while an asynchronous solve is in flight,
 * and while a constraint table is bound -- as mpc_set_agent_constraints is while a rate table is bound (the kernels have
 * no form that takes both; a handle's own constraint data works).
 * The closed loops carry u_{-1} themselves.  With a rate table bound, mpc_closed_loop, mpc_closed_loop_event,
 * mpc_closed_loop_track and mpc_closed_loop_traffic need one row per agent (P == B, MPC_E_ARG otherwise; the index being
 * 0 .. B-1 is the caller's to ensure, the Python front end does) and, behind the solve of a step and before the plant
 * moves or the plan shifts, write the input about to be applied into columns 2 and 3 of row index[b]: U[b][0..1]
 * (mpc_closed_loop, _traffic) or U[b][2 held .. 2 held + 1] (_event, _track; held = 0 for an agent that has just
 * re-planned).  That is, bit for bit, the host loop of the public calls in which the caller writes those two columns
 * between the solve and the rollout; the table holds the last applied inputs when the loop returns. */
#define MPC_NRATE 4
int mpc_default_rates(const mpc_config *cfg, double *row);
int mpc_set_agent_rates(mpc_handle *h, const double *table, int P, const int32_t *index, int B);

/* Risk-field cost: soft obstacle potentials per agent and stage -- a sixth table of P rows in device memory and one row
 * index per agent; like the disc table its data varies with the stage.  One row, all doubles:
 * [N][MPC_NFIELD][MPC_NFSRC], MPC_FIELD_ROW(N) of them.  One source is [cx, cy, c, s, A, kx, ky, alpha]: a skewed
 * anisotropic Gaussian (the `dnf` part of the reference's driving-risk potential field) of height A around (cx, cy);
 * (c, s) are the cosine and sine of the source's own frame, kx = 1 / (2 sigma_x^2) acts along the frame and ky across it,
 * alpha is the skew along it (in the reference (v - v_obs) / 5; here frozen into the data).  With (x, y) the position at
 * the end of stage k (x_{k+1}, where every stage term is taken), stage k's cost -- behind the move penalty and before the
 * ALM terms -- gets its sources, and the stage's state gradient their derivative, every operation rounded on its own and
 * in this order, source j = 0 before j = 1:
 *     dx = x - cx,  dy = y - cy,  a = (c dx) + (s dy),  l = (c dy) - (s dx)
 *     E = ((kx a) a + (ky l) l) + alpha a,   V = A exp(-E),   L_k = L_k + V
 *     ga = -(V (2 (kx a) + alpha)),  gl = -(V (2 (ky l)))
 *     dL/dx_k[0] = dL/dx_k[0] + ((c ga) - (s gl)),   dL/dx_k[1] = dL/dx_k[1] + ((s ga) + (c gl))
 * psi stays the sum of the stage costs in stage order; the adjoint recursion carries the state gradient like any other.
 * A source with A == 0 is skipped: it adds nothing, not even a signed zero -- that is how "no obstacle at this stage" is
 * said, and a table of zeros gives the bits of the call without a table.  exp is the device library's, full range, one
 * out-of-line body for the four evaluation routes (K1b, the fused K1b + K1c kernel, the wave evaluation, the persistent
 * kernel), which call one device function: a request gets the same bits whichever serves it.  It is a cost, not a
 * constraint: no multiplier, and the inner problem stays feasible whatever the sources are.
 * The table is read by mpc_eval_cost_grad(_wave), mpc_solve_batch(_async), mpc_solve_active and the closed loops (which
 * read it as it is bound -- obstacles standing on the track: stage k of every re-plan reads entry k of the agent's row);
 * mpc_stage_cost, mpc_rhs, mpc_rollout and mpc_prox_step do not read it.  Handles of MPC_CONSTR_NONE, _STATE_SQ and _LANE
 * take it, with the handle's own constraint data (a lane band and soft obstacles in one solve); beside a rate table the
 * two terms add up.
 * mpc_default_fields (host only): a row of zeros, MPC_FIELD_ROW(cfg->N) doubles.
 * mpc_set_agent_fields: the semantics of the other tables.  table == NULL unbinds; bound, the calls above use row
 * index[b] for agent b and return MPC_E_ARG for a batch size other than B; bound beside other tables it is for the same
 * B.  table [P][MPC_FIELD_ROW(N)] and index [B] are DEVICE memory of the caller, read at every call: rows may be
 * rewritten in place between calls.  At P == B = 65 536, N = 20 the table is 168 MB.  The P rows are checked once, at bind
 * time: every value finite, A >= 0, kx >= 0, ky >= 0, and alpha != 0 only with kx > 0 (or the skew is unbounded); index
 * ranges are the caller's to check (the Python front end does).  Refused (MPC_E_ARG) while an asynchronous solve is in
 * flight, on a handle of MPC_CONSTR_DISCS (there an obstacle is a disc), and while a constraint table is bound -- as
 * mpc_set_agent_constraints is while a field table is bound (the kernels have no form that takes both).
 * mpc_fields_from_plans: the gather for inter-agent avoidance, asynchronous on `stream`.  X [B][N][nx] is what
 * mpc_rollout wrote for the agents' current plans, opp [B][MPC_NFIELD] (int32) the opponents of agent b (< 0 or >= B:
 * none; MPC_NFIELD == MPC_NDISC, so an opp of mpc_opponents_from_plans serves), shape [B][4] = [A, kx, ky, gain] agent b
 * AS AN OBSTACLE; table [B][MPC_FIELD_ROW(N)] receives, for o = opp[b][j],
 *     table[b][k][j] = [X[o][k][0], X[o][k][1], cos X[o][k][2], sin X[o][k][2], shape[o][0], shape[o][1], shape[o][2],
 *                       shape[o][3] * (X[b][k][3] - X[o][k][3])]
 * -- cos and sin by the device's sincos, the subtraction and the product each rounded on its own; column 3 is v on the
 * kinematic model and vx on the Pacejka model -- or eight zeros where there is no opponent.  shape is device data and is
 * not checked, as radius is not.  All four are device memory.
 * mpc_closed_loop_traffic_field: mpc_closed_loop_traffic with soft obstacles -- its arguments and its steps, `shape`
 * beside `radius` (which still drives the selection and traj_clear), step 3 being table = mpc_fields_from_plans(X, opp,
 * shape), and `table` the FIELD table currently bound, with P == B rows.  On a handle of any constr_mode except
 * MPC_CONSTR_DISCS (lambda may be NULL where m == 0). */
#define MPC_NFIELD 2
#define MPC_NFSRC 8
#define MPC_FIELD_ROW(N) (MPC_NFIELD * MPC_NFSRC * (N))
int mpc_default_fields(const mpc_config *cfg, double *row);
int mpc_set_agent_fields(mpc_handle *h, const double *table, int P, const int32_t *index, int B);
int mpc_fields_from_plans(mpc_handle *h, int B, const double *X, const int32_t *opp, const double *shape, double *table,
                          void *stream);
int mpc_closed_loop_traffic_field(mpc_handle *h, int B, int T, int shift, int G, const double *radius, const double *shape,
                                  double reach, double *x, const double *cl, const int32_t *cl_index, double *U,
                                  double *lambda, double *table, double *traj_x, double *traj_u, int32_t *traj_opp,
                                  double *traj_clear, int32_t *fail_count, double *stats, void *stream);

/* Road cost: a per-stage lane target, soft road edges and a per-stage speed target -- a seventh table of P rows in device
 * memory and one row index per agent; like the disc and field tables its data varies with the stage.  One row, all
 * doubles: [N][MPC_NROAD], MPC_ROAD_ROW(N) of them.  A stage's entry is [off, w_off, lo, w_lo, hi, w_hi, v_tgt, w_v]:
 * the target-lane well w_off (e - off)^2 and the road boundary w_lo (e - lo)^2 below lo, w_hi (e - hi)^2 above hi, 0
 * between (the road part of the reference's driving potential, restated in this project's frame), and w_v (sp - v_tgt)^2
 * on the speed.  e is the signed lateral offset from the centerline, exactly the lane band's expression
 * (MPC_CONSTR_LANE): POSITIVE TO THE RIGHT of the direction of travel -- on a line y = 0.5 driven towards +x,
 * e = -(y - 0.5).  With (nx, ny) the nearest centerline point of the position at the end of stage k, (qx, qy) its
 * successor and x the state at the end of the stage (x_{k+1}, where every stage term is taken), stage k's cost -- behind
 * the risk field (on a handle of MPC_CONSTR_DISCS: behind the move penalty) and before the ALM terms -- gets, every
 * operation rounded on its own and in this order:
 *     wx = qx - nx,  wy = qy - ny,  nrm = sqrt(wx wx + wy wy),  e = ((x[0] - nx) wy - (x[1] - ny) wx) / nrm,  de = 0
 *     w_off != 0:                  t = e - off,  a = w_off t,  L_k = L_k + a t,  de = de + 2 a
 *     w_lo != 0 and q = e - lo < 0:              a = w_lo q,   L_k = L_k + a q,  de = de + 2 a
 *     w_hi != 0 and p = e - hi > 0:              a = w_hi p,   L_k = L_k + a p,  de = de + 2 a
 *     gradient request, any of the three weights != 0:
 *         dL/dx_k[0] = dL/dx_k[0] + (de wy) / nrm,   dL/dx_k[1] = dL/dx_k[1] - (de wx) / nrm
 *     w_v != 0:  ev = sp - v_tgt (sp as in the stage cost: x[3], or sqrt(x[3] x[3] + x[4] x[4]) on the Pacejka model),
 *                a = w_v ev,  L_k = L_k + a ev
 *                gradient request: kinematic  dL/dx_k[3] = dL/dx_k[3] + 2 a;
 *                                  Pacejka    dL/dx_k[3] = dL/dx_k[3] + ((2 a) x[3]) / sp,  dL/dx_k[4] likewise with x[4]
 * psi stays the sum of the stage costs in stage order; the adjoint recursion carries the state gradient like any other.
 * A part whose weight is 0 is skipped by a branch: it adds nothing, not even a signed zero, so a table of zero weights
 * gives the bits of the call without a table, whatever its other words are; with no lateral weight set e and nrm are not
 * computed.  Where two neighbouring centerline points coincide (nrm == 0) the term is what the lane band is there today:
 * e = 0 / 0 is not a number, and so is the cost of every stage that lands there with a lateral weight set; a centerline
 * without repeated points never gets there.  Likewise on the Pacejka model at sp == 0 with w_v != 0: the speed gradient
 * divides by sp and is 0 / 0 there, as the stage cost's own speed term is.  One device function (road_term) serves the four evaluation routes (K1b,
 * the fused K1b + K1c kernel, the wave evaluation, the persistent kernel): a request gets the same bits whichever serves
 * it.  It is a cost, not a constraint: no multiplier; the step kernel, the prox and the constraint bounds do not know it.
 * So it is allowed on handles of EVERY constr_mode -- on a handle of MPC_CONSTR_DISCS "keep out of these discs and stay
 * on the road" is one solve -- beside the parameter, bounds, rate and field tables and beside the disc table; the terms
 * add up.  The table is read by mpc_eval_cost_grad(_wave), mpc_solve_batch(_async), mpc_solve_active and the closed loops
 * (which read it as it is bound: stage k of every re-plan reads entry k of the agent's row); mpc_stage_cost, mpc_rhs,
 * mpc_rollout and mpc_prox_step do not read it.
 * mpc_default_roads (host only): a row of zeros, MPC_ROAD_ROW(cfg->N) doubles.
 * mpc_set_agent_roads: the semantics of the other tables.  table == NULL unbinds; bound, the calls above use row index[b]
 * for agent b and return MPC_E_ARG for a batch size other than B; bound beside other tables it is for the same B.  table
 * [P][MPC_ROAD_ROW(N)] and index [B] are DEVICE memory of the caller, read at every call: rows may be rewritten in place
 * between calls.  The P rows are checked once, at bind time: every value finite, no weight negative, and lo <= hi on
 * every stage where w_lo and w_hi are both non-zero; index ranges are the caller's to check (the Python front end does).
 * Refused (MPC_E_ARG) while an asynchronous solve is in flight, and while a constraint table is bound -- as
 * mpc_set_agent_constraints is while a road table is bound (the kernels have no form that takes both).
 * mpc_roads_from_script: rows that move in time, asynchronous on `stream`.  script [Ps][Lt][MPC_NROAD] holds one sample
 * per Ts, sidx [B] (int32, 0 <= sidx[b] < Ps: the caller's to check) one script row per agent; row b of table
 * [B][MPC_ROAD_ROW(N)] receives, for k < N, sample min(ti + k, Lt - 1) of script row sidx[b] -- or sample (ti + k) mod Lt
 * with wrap != 0: the time rule of mpc_discs_from_obstacles.  A plain copy; the samples are not checked (the binder
 * checked the table's rows once, the script's are the caller's to keep valid).  Although the copy reads no bound table,
 * B must be the B of whatever tables are bound (MPC_E_ARG otherwise), as for mpc_discs_from_obstacles.  table may be the bound road table: a host
 * loop of mpc_roads_from_script, mpc_solve_batch and mpc_rollout (or of mpc_roads_from_script and mpc_closed_loop with
 * T = 1) advances a lane change or a speed profile through a closed loop without uploading B x N x 8 doubles per step.
 * All three are device memory.  No closed loop performs this gather itself, and profiles are indexed by time, not by
 * track position. */
#define MPC_NROAD 8
#define MPC_ROAD_ROW(N) (MPC_NROAD * (N))
int mpc_default_roads(const mpc_config *cfg, double *row);
int mpc_set_agent_roads(mpc_handle *h, const double *table, int P, const int32_t *index, int B);
int mpc_roads_from_script(mpc_handle *h, int B, int Lt, int wrap, int ti, const double *script, const int32_t *sidx,
                          double *table, void *stream);

/* a-1(car_dynamics.py:93-132 / dynamics.py:67-119,:144-173): dx[B][nx] = f(x[B][nx], u[B][2]) */
int mpc_rhs(mpc_handle *h, int B, const double *x, const double *u, double *dx, void *stream);

/* a-2/a-3 (car_dynamics.py:134-147,:159-166 simulate/mapaccum): X[B][Nsim][nx] = x_1..x_Nsim;
 * U is [B][2*Nsim].  Nsim = 1 is the plant step of main.py:145. */
int mpc_rollout(mpc_handle *h, int B, int Nsim, const double *x0, const double *U, double *X,
                void *stream);

/* f-2 (car_dynamics.py:185-190, the 98-candidate scan per stage): prepares the exact pruned
 * nearest-point search for the centerline table cl [C][2S], on `stream`: a grid of index ranges per
 * row -- every cell holds the range [lo, hi] guaranteed to contain the scan's answer for any point of
 * the cell (not built for a table of more than 1 024 rows).  Later calls that are handed the SAME table
 * pointer (mpc_solve_batch, mpc_eval_cost_grad*, mpc_stage_errors, mpc_closed_loop) use the search
 * mpc_set_nearest_blocks selects; any other table takes the full scan.  The index found is the same
 * whichever runs, bit for bit.  Call it again whenever the table's contents change.
 * mpc_set_nearest_blocks(h, mode): 0 full scan (environment MPC_NEAREST_SCAN), 2 grid (default;
 * measured 4.8 % faster solves: DESIGN.md 8).  Mode 1, the block-box search, was removed: MPC_E_ARG. */
int mpc_centerline_blocks(mpc_handle *h, const double *cl, int C, void *stream);
int mpc_set_nearest_blocks(mpc_handle *h, int on);

/* a-4/a-5 (car_dynamics.py:174-228): pose[B][3] = [x, y, phi] -> err[B][3] = [cte, heading_error,
 * pos_error], idx[B] = nearest index (idx may be NULL).  Diagnostics of main.py:122-133. */
int mpc_stage_errors(mpc_handle *h, int B, const double *pose, const double *cl,
                     const int32_t *cl_index, double *err, int32_t *idx, void *stream);

/* a-6 (car_dynamics.py:230-258 L_cost): out[B] = stage cost of (x[B][nx], u[B][2]) */
int mpc_stage_cost(mpc_handle *h, int B, const double *x, const double *u, const double *cl,
                   const int32_t *cl_index, double *out, void *stream);

/* a-6..a-9, kernel K1: psi[B] = f(U) + 1/2 dist_Sigma^2(g(U)+y/Sigma, D); grad[B][2N] (NULL: cost
 * only); yhat[B][m] (NULL ok).  y, Sigma [B][m] are ignored when m == 0.
 * Replaces the CasADi-generated f / grad_f / g / grad_g_prod that alpaqa calls (main.py:54). */
int mpc_eval_cost_grad(mpc_handle *h, int B, const double *x0, const double *cl,
                       const int32_t *cl_index, const double *U, const double *y,
                       const double *Sigma, double *psi, double *grad, double *yhat, void *stream);

/* the same evaluation by the wave-per-agent code of the persistent solve kernel (one wavefront per
 * agent: wide rollout, stage k on lane k, adjoint on one lane) -- bit-identical results */
int mpc_eval_cost_grad_wave(mpc_handle *h, int B, const double *x0, const double *cl,
                            const int32_t *cl_index, const double *U, const double *y,
                            const double *Sigma, double *psi, double *grad, double *yhat, void *stream);

/* two points of every agent in one trip of that code: the evaluation at U (psi; grad, NULL: cost only; yhat) on one
 * half of the wavefront and the gradient at U2 (grad2[B][2N]) on the other, as a trip of the persistent kernel that
 * carries a speculative gradient runs them -- bit-identical to two calls of mpc_eval_cost_grad.  Kinematic model,
 * nfe = 4, N <= 32. */
int mpc_eval_cost_grad_wave2(mpc_handle *h, int B, const double *x0, const double *cl,
                             const int32_t *cl_index, const double *U, const double *U2, const double *y,
                             const double *Sigma, double *psi, double *grad, double *grad2, double *yhat, void *stream);

/* a-10, kernel K2: forward-backward step. p = clamp(-gamma*grad, lb-x, ub-x), xhat = x+p;
 * out[B][2] = [||p||^2, grad'p].  gamma[B]. */
int mpc_prox_step(mpc_handle *h, int B, const double *x, const double *grad, const double *gamma,
                  double *xhat, double *p, double *out, void *stream);

/* a-11, kernel K3: masked L-BFGS two-loop.  S,Y [B][M][n] history (row i of agent b is pair i),
 * idx[B] = next write slot, full[B] = ring full flag, mask[B][n] (1 = index in J), q[B][n] inout,
 * ok[B] out (0 when no valid pair: q untouched). */
int mpc_lbfgs_apply(mpc_handle *h, int B, const double *S, const double *Y, const int32_t *idx,
                    const int32_t *full, const double *mask, double *q, int32_t *ok, void *stream);

/* a-8..a-13: the batched solve.  U [B][2N] and lambda [B][m] are warm start in / solution out
 * (controller.py:57); stats [B][MPC_NSTATS].  Replaces `self.solver(self.problem, self.U, self.lam)`. */
int mpc_solve_batch(mpc_handle *h, int B, const double *x0, const double *cl,
                    const int32_t *cl_index, double *U, double *lambda, double *stats,
                    void *stream);

/* The same solve without holding the caller's thread: the round loop (launches and counter polls, host
 * code) runs on a worker thread of the handle; mpc_solve_wait blocks until the solve is complete (all
 * results in the caller's buffers, the stream drained) and returns its code.  One solve in flight per
 * handle; no other call on the handle between the two.  ("async on the given stream".) */
int mpc_solve_batch_async(mpc_handle *h, int B, const double *x0, const double *cl,
                          const int32_t *cl_index, double *U, double *lambda, double *stats,
                          void *stream);
int mpc_solve_wait(mpc_handle *h);

/* f-1 (main.py:121-146): T closed-loop steps with states, controls and warm starts resident on the
 * device: per step one mpc_solve_batch (whose round loop is HOST code: launches and counter polls, like
 * any solve) followed by one kernel that applies u0 and advances the plant with f_d.  Data never leaves
 * the device; control returns to the host once per round window, as in every solve.
 * x [B][nx] inout; U, lambda warm start inout; traj_x [B][T][nx], traj_u [B][T][2] (NULL ok);
 * shift != 0 shifts the warm start by one stage (the reference does not: controller.py:57).
 * fail_count[B] int32 accumulates status != Converged (controller.py:64), NULL ok. */
int mpc_closed_loop(mpc_handle *h, int B, int T, int shift, double *x, const double *cl,
                    const int32_t *cl_index, double *U, double *lambda, double *traj_x,
                    double *traj_u, int32_t *fail_count, double *stats, void *stream);

/* The masked solve: active [B] is a DEVICE mask; the agents with active[b] != 0 are solved exactly as mpc_solve_batch
 * solves them (warm start in, solution out, the same bits), and every byte of U, lambda and stats that belongs to
 * another agent is left as it was.  *n_active (HOST int, NULL ok) receives the number of agents solved; none active:
 * no solver kernel runs, MPC_OK.  By compaction: an index-ascending list of the active agents (two passes, no
 * atomics: reproducible), their x0 / U / lambda / cl_index / parameter-row index gathered into buffers of the handle,
 * the solve of mpc_solve_batch on those rows, U / lambda / stats scattered back.  With a parameter table bound B is the
 * bound batch.  Blocking, like mpc_solve_batch. */
int mpc_solve_active(mpc_handle *h, int B, const int32_t *active, const double *x0, const double *cl,
                     const int32_t *cl_index, double *U, double *lambda, double *stats, int32_t *n_active,
                     void *stream);

/* The trigger of the event-triggered loop, on its own (asynchronous on `stream`): e = x - xhat, the heading component
 * (index 2) reduced by e -= 2 pi rint(e / 2 pi); dev2[b] = sum_i w_i e_i^2 in index order, each operation rounded on
 * its own; fire[b] = held[b] < 0 || held[b] >= max_hold || dev2[b] >= thr^2 (a non-finite dev2 fires; thr = 0 always
 * fires; thr = +inf leaves the hold limit alone).  x, xhat [B][nx], held [B] int32, fire [B] int32, dev2 [B] (NULL ok):
 * DEVICE memory; w [nx] is a HOST array.  MPC_E_ARG unless thr >= 0 and 1 <= max_hold <= N. */
int mpc_trigger_eval(mpc_handle *h, int B, const double *x, const double *xhat, const int32_t *held,
                     const double *w, double thr, int max_hold, double *dev2, int32_t *fire, void *stream);

/* Event-triggered closed loop: an agent keeps applying the plan it holds until the plant has drifted from the plan's
 * own prediction by thr or more (the trigger above) or max_hold stages of it have been applied; only then is it solved
 * again (the masked solve above).  Per-agent state: the plan U as last solved; held [B] int32 inout, the stages of it
 * already applied (-1: no plan yet); the nominal state xhat [B][nx], owned by the handle.  Step t:
 *   1. fire = trigger(x, xhat, held);
 *   2. shift != 0: a firing agent's plan is shifted in place by `held` stages, the last stage repeated into the tail;
 *   3. the firing agents are solved (warm start U, lambda), then held = 0, xhat = x;
 *   4. fail_count [B] accumulates status != Converged, solve_count [B] the solves, of the agents solved at this step;
 *   5. every agent applies u = U[2 held .. 2 held + 1]: x <- f_d(x, u) on the plant's row (+ disturbance[b][t][:] when
 *      that pointer is not NULL: [B][T][nx], the caller's data -- the library draws no random numbers),
 *      xhat <- f_d(xhat, u) on the controller's row, held += 1; traj_x [B][T][nx], traj_u [B][T][2] and
 *      solved [B][T] (uint8: the agent was solved at step t) are written (each NULL ok, as solve_count, fail_count).
 * On return U is the plan as last solved and held says how far it is consumed: a later call on the same handle and
 * batch continues from there (on a handle that holds no nominal states for this batch every agent is solved at the
 * first step).  stats [B][MPC_NSTATS] (NULL ok) holds each agent's most recent solve.  thr = 0 is mpc_closed_loop,
 * bit for bit.  Blocking. */
int mpc_closed_loop_event(mpc_handle *h, int B, int T, int shift, const double *w, double thr, int max_hold,
                          double *x, const double *cl, const int32_t *cl_index, double *U, double *lambda,
                          int32_t *held, const double *disturbance, double *traj_x, double *traj_u,
                          uint8_t *solved, int32_t *solve_count, int32_t *fail_count, double *stats, void *stream);

/* Lap driving: per-agent centerline windows on long and closed tracks.  A centerline row is S points and the nearest
 * point is searched among candidates 0 .. S-2 of ONE row: an agent that reaches the end of its row sticks there.  A track
 * is therefore cut into overlapping windows, each an ordinary centerline row, and an agent's row is re-selected on the
 * device whenever it re-plans; K1b, the grid of index ranges and every solver kernel see what they always saw.
 *
 * Track table: track [K][2L], each row flat [x_0..x_{L-1}, y_0..y_{L-1}] like a centerline row; a CLOSED track does not
 * repeat its first point at the end.  With stride w, window r of track k is row k*R + r of win [K*R][2S] and holds track
 * points r*w + i, i < S -- on a closed track the point index is taken mod L and R = ceil(L / w); on an open track
 * R = (L - S) / w + 1 (integer division).  L >= S in both cases.
 *
 * The rule, for an agent on row k*R + r whose nearest index on that row is i (integers only; the one floating-point
 * decision is the nearest index):
 *     open:    p = r*w + i - lead,            r' = min(max(floor(p / w), 0), R - 1)   (floor towards minus infinity)
 *     closed:  p = (r*w + i - lead) mod L,    r' = p / w                             (0 <= p < L)
 *     new row = k*R + r',   pos = r*w + i  (mod L on a closed track): the track point the agent stands at.
 * Where nothing is clamped the agent's nearest index on its new row lies in [lead, lead + w): `lead` points of the track
 * behind it, S - lead - w or more ahead.
 *
 * mpc_track_init (host only): checks K >= 1, L >= S, stride >= 1, 0 <= lead <= S - 2 and that K * R fits an int32
 *   (MPC_E_ARG otherwise) and fills *t, R included.  The other calls refuse a track that is not what it gives for the
 *   handle's S.
 * mpc_track_windows: win from track, a pure gather, asynchronous on `stream`: every word of win is a copy of a word of
 *   track.  The caller then prepares the search tables for win once (mpc_centerline_blocks(h, win, K*R, stream)).
 *   GRID LIMIT: the grid of index ranges is built for at most 1 024 rows (256 KB each); a window table with K*R above that
 *   takes the full scan in every call -- the same results, slower.  The caller chooses the stride accordingly.
 * mpc_track_select: x [B][nx] (only x[b][0], x[b][1] are read), cl_index [B] inout, pos [B] out (NULL ok).  The nearest
 *   index is the one K1b will find for that row: the search mpc_set_nearest_blocks selects with the tables
 *   mpc_centerline_blocks built for `win`, the full scan if there are none -- the same index, bit for bit.  An agent with
 *   active[b] == 0 (active NULL: all are active), one whose x or y is not finite and one whose cl_index is not a row of
 *   the table is not written (neither cl_index nor pos).  Asynchronous on `stream`.
 * mpc_track_locate: the first placement.  a = nearest index by the same rule on the agent's WHOLE track row
 *   track_index[b] (NULL: track 0): candidates 0 .. L-2, first minimum, the same squared-distance expression; then the
 *   rule above with r*w + i replaced by a.  An agent whose track_index is not a track of the table is not written.
 *   Asynchronous on `stream`.
 * mpc_closed_loop_track: mpc_closed_loop_event (every argument of it, cl = win, cl_index NOT const and not NULL) with one
 *   step between 1 and 2: the FIRING agents re-select their row (mpc_track_select with active = fire, on the plant state
 *   x); an agent that holds its plan keeps the row the plan was solved on.  traj_row [B][T] (NULL ok) is the row in force
 *   at step t.  thr = 0 re-selects and solves everybody at every step.  A later call continues from cl_index, held and the
 *   nominal states, as the event loop does.  The caller builds win and its search tables once, before the loop: the loop
 *   builds nothing.  On a one-window track it is mpc_closed_loop_event on that row, bit for bit.  Blocking.
 * All of them are refused (MPC_E_ARG) while an asynchronous solve is in flight; with a parameter, bounds or constraint
 * table bound, the calls that take B return MPC_E_ARG for a batch size other than the bound one. */
typedef struct mpc_track { int32_t K, L, stride, lead, closed, R; } mpc_track;
int mpc_track_init(mpc_track *t, const mpc_config *cfg, int K, int L, int stride, int lead, int closed);
int mpc_track_windows(mpc_handle *h, const mpc_track *t, const double *track, double *win, void *stream);
int mpc_track_locate(mpc_handle *h, const mpc_track *t, int B, const double *x, const double *track,
                     const int32_t *track_index, int32_t *cl_index, void *stream);
int mpc_track_select(mpc_handle *h, const mpc_track *t, int B, const double *x, const double *win,
                     const int32_t *active, int32_t *cl_index, int32_t *pos, void *stream);
int mpc_closed_loop_track(mpc_handle *h, int B, int T, int shift, const double *w, double thr, int max_hold,
                          double *x, const double *win, int32_t *cl_index, double *U, double *lambda,
                          int32_t *held, const double *disturbance, double *traj_x, double *traj_u,
                          uint8_t *solved, int32_t *solve_count, int32_t *fail_count, double *stats, void *stream,
                          const mpc_track *trk, int32_t *traj_row);

/* Scripted moving obstacles: obstacle TRAJECTORIES per scene, the selection of the ones that matter to each agent, decided
 * on the device, and the closed loop around it.  Scenes are the traffic loop's: contiguous blocks of G agents, agent b in
 * scene b / G, 1 <= G <= MPC_SCENE_MAX and B % G == 0.  Every scene has K scripted obstacles, 1 <= K <= MPC_SCENE_MAX, each
 * of Lt >= 1 samples, one per Ts of the handle, shared by the scene's G agents: obs [B / G][K][Lt][W], doubles in DEVICE
 * memory of the caller.  W = 3 on a handle of MPC_CONSTR_DISCS, a sample being (cx, cy, r); W = MPC_NFSRC on every other
 * handle, a sample being a whole risk source (cx, cy, c, s, A, kx, ky, alpha) -- the caller scripts frame and skew.  A
 * sample is ABSENT iff r == 0 (discs) or A == 0 (fields): "not there yet", "gone".  The sample of time i >= 0, in
 * integers: wrap ? i mod Lt : min(i, Lt - 1) -- a script that ends leaves its obstacle standing at the last sample, a
 * periodic one serves an obstacle circling a closed track.  obs is device data and is not checked, as radius is not
 * (the Python front end's obstacle_tracks applies the row rules of mpc_set_agent_discs / _fields).
 * mpc_obstacles_select: X [B][Nst][nx] as mpc_rollout writes it (Nst = 1 with X = x: the states as they are); stage k is
 * compared with sample ti + k of every obstacle o < K of b's scene.  The rule, every operation rounded on its own (a host
 * loop in IEEE doubles gets the same bits), over the stages k < Nst whose sample is present:
 *     dx = X[b][k][0] - cx, dy = X[b][k][1] - cy, g_k = (dx dx + dy dy) - r2,   c(b, o) = min_k g_k
 * with r2 = r r for discs and 0 for fields -- the disc expression and the rule of mpc_opponents_from_plans, operand for
 * operand.  A pair with a g_k that is not finite is out; an obstacle with no present sample in the window is no
 * candidate; o is a candidate iff c(b, o) < reach reach (reach >= 0; +inf: all).  Selected are the MPC_NDISC candidates
 * smallest in the lexicographic order (c, o), ties to the smaller o.  sel [B][MPC_NDISC] (int32, out) holds the obstacle's
 * index WITHIN THE SCENE, an unused slot -1 with clear = +inf; clear [B][MPC_NDISC] (out) may be NULL.  No atomics.
 * Asynchronous on `stream`.  MPC_E_ARG before any launch: G or K outside [1, MPC_SCENE_MAX], B % G != 0, Lt < 1, ti < 0,
 * ti + Nst not an int32, Nst < 1, reach negative or NaN, NULL X, obs or sel, an asynchronous solve in flight, and, with
 * tables bound, a B other than the bound one.
 * mpc_discs_from_obstacles (only on a handle of MPC_CONSTR_DISCS) and mpc_fields_from_obstacles (on every other): the
 * gather, asynchronous on `stream`.  table [B][MPC_DISC_ROW(N)] or [B][MPC_FIELD_ROW(N)] receives, for k < N,
 *     table[b][k][j] = obs[b / G][sel[b][j]][sample(ti + k)]     (W words)
 * and W zeros where sel[b][j] is outside [0, K) and where the sample is absent (its other words are never copied: junk
 * behind r == 0 cannot reach a constraint).  Every word written is a copy of an input word or zero.  The refusals of the
 * selection that apply (ti + N in place of ti + Nst), NULL sel or table, and the handle's constr_mode.
 * mpc_closed_loop_obstacles: T closed-loop steps among the scripted obstacles, on a handle of any constr_mode.  Blocking;
 * the arguments it shares with mpc_closed_loop_traffic mean what they mean there.  `table` must be the bound disc table
 * (MPC_CONSTR_DISCS) or the bound field table (every other mode) with P == B rows, index 0 .. B-1 (MPC_E_ARG otherwise);
 * with a rate table bound it needs one row per agent as in the other loops.  Step t, every numbered launch being the one
 * the public call of that name makes:
 *   0. only with trk != NULL: mpc_track_select(x, cl as win, active = NULL, cl_index) -- lap driving among moving
 *      obstacles, everybody re-selecting its window at every step (mpc_closed_loop_track at thr = 0 does); with
 *      trk == NULL cl_index is read only and may be NULL
 *   1. X = mpc_rollout(x, U), N stages, into a buffer of the handle
 *   2. sel = mpc_obstacles_select on X with ti = t0 + t + 1, Nst = N; traj_sel [B][T][MPC_NDISC] records it (NULL ok)
 *   3. table = the gather of the handle's kind with the same ti
 *   4. mpc_solve_batch; U and lambda are warm starts, lambda is NOT re-slotted when the selection changes
 *   5. the rate table's u_prev write and the plant step of mpc_closed_loop, as the traffic loop launches them
 *   6. traj_clear [B][T] (NULL ok) = slot 0 of `clear` of the selection on the NEW states (Nst = 1, ti = t0 + t + 1,
 *      reach = +inf): the realised clearance at time t + 1; +inf when nothing is present
 * t0 >= 0 lets a later call continue the script: two calls of T steps (the second with t0 + T and what the first
 * returned) are one of 2 T.  Also MPC_E_ARG: T < 0, t0 < 0, t0 + T + N not an int32.  Nothing but the solve's own polls
 * returns to the host. */
int mpc_obstacles_select(mpc_handle *h, int B, int G, int K, int Lt, int wrap, int ti, int Nst, const double *X,
                         const double *obs, double reach, int32_t *sel, double *clear, void *stream);
int mpc_discs_from_obstacles(mpc_handle *h, int B, int G, int K, int Lt, int wrap, int ti, const double *obs,
                             const int32_t *sel, double *table, void *stream);
int mpc_fields_from_obstacles(mpc_handle *h, int B, int G, int K, int Lt, int wrap, int ti, const double *obs,
                              const int32_t *sel, double *table, void *stream);
int mpc_closed_loop_obstacles(mpc_handle *h, int B, int T, int shift, int G, int K, int Lt, int wrap, int t0,
                              const double *obs, double reach, double *x, const double *cl, int32_t *cl_index,
                              double *U, double *lambda, double *table, double *traj_x, double *traj_u,
                              int32_t *traj_sel, double *traj_clear, int32_t *fail_count, double *stats, void *stream,
                              const mpc_track *trk);

/* Event-triggered holding among scripted obstacles: mpc_closed_loop_event's trigger watches the car alone, and an obstacle
 * that appears does not move the plant off its plan; these three calls add the trigger that watches the obstacles.  It is
 * time-aligned: stage held + k of a held plan meets sample ti + k of the scripts.
 * mpc_rollout_held: X [B][N][nx] (out), the states agent b reaches from x[b] by going on applying the plan U[b] ([B][2N])
 * of which it has applied held[b] stages: with k_b = min(max(held[b], 0), N - 1), X[b][j] is the state after the inputs
 * u_{min(k_b + i, N - 1)}, i = 0 .. j -- the last input repeated into the tail, the index rule of the in-place shift of
 * mpc_closed_loop_event.  On the controller's parameter row, as mpc_rollout.  Bit for bit mpc_rollout(x, the shifted U);
 * held <= 0 is mpc_rollout(x, U).  One thread per agent, asynchronous on `stream`.  MPC_E_ARG: a NULL buffer, with tables
 * bound a B other than the bound one, an asynchronous solve in flight.
 * mpc_obstacle_trigger: the obstacle rule, pure -- it shifts no plan and rewrites no table.  The scene arguments are
 * mpc_obstacles_select's; X [B][N][nx] is mpc_rollout_held's; sel_plan [B][MPC_NDISC] (int32) holds the tracks the held
 * plan was solved against (-1: none).  The selection of mpc_obstacles_select runs for agent b over the stages its plan
 * still holds, j < N - k_b, and no others (the repeated tail was never constrained and does not fire the rule), stage j
 * against sample ti + j: sel_chk [B][MPC_NDISC] and clear_chk [B][MPC_NDISC] (out; slot 0 is the smallest c < reach^2,
 * +inf if there is none).  Then, per agent, why[b] (uint8, out, NULL ok):
 *     bit 0 (1)  fire_in[b] != 0 (fire_in [B] int32, e.g. mpc_trigger_eval's; NULL: none)
 *     bit 1 (2)  held[b] > 0, watch & 1 and !(clear_chk[b][0] >= clear_thr): the plan comes too close
 *     bit 2 (4)  held[b] > 0, watch & 2 and some sel_chk[b][j] >= 0 is not a member of {sel_plan[b][0], sel_plan[b][1]}:
 *                a new obstacle (set membership: a change of order is none)
 * and fire_out[b] = why[b] != 0 (int32, out; may be fire_in).  clear_thr is in the units of the clearance: on a handle of
 * MPC_CONSTR_DISCS g = d^2 - r^2, and a solved plan rides g = 0 to within alm_delta, so a useful clear_thr is slightly
 * negative; on every other handle r2 = 0 and clear_thr is a squared distance.  Asynchronous on `stream`.  MPC_E_ARG before
 * any launch: everything mpc_obstacles_select refuses (Nst = N), clear_thr > reach^2 (slot 0 would not see it) or NaN,
 * watch outside [0, 3], a NULL X, held, sel_plan, sel_chk, clear_chk or fire_out.
 * mpc_closed_loop_obstacles_event: mpc_closed_loop_obstacles in which an agent keeps applying the plan it holds.  The
 * arguments are those of mpc_closed_loop_event (w, thr, max_hold, held, disturbance, solved, solve_count) and of
 * mpc_closed_loop_obstacles (the scene, t0, table, traj_sel, traj_clear, trk), clear_thr and watch as above, sel_plan
 * [B][MPC_NDISC] (in/out) and traj_why [B][T] (uint8, NULL ok).  Blocking.  Step t, ti = t0 + t + 1, every launch being
 * the one the public call of that name makes:
 *   1. fire = mpc_trigger_eval(x, xhat, held) -- no plan is shifted yet; a handle that has no nominal states for this B
 *      fires everybody at its first step, as in mpc_closed_loop_event
 *   2. X = mpc_rollout_held(x, U, held)
 *   3. fire, traj_why[.][t] = mpc_obstacle_trigger(X, held, sel_plan, fire_in = fire) at ti
 *   4. shift != 0: the plans of the firing agents with held > 0 are shifted in place by k_b stages
 *   5. trk != NULL: mpc_track_select(x, active = fire) -- the firing agents re-select their window
 *   6. sel = mpc_obstacles_select(X, ti, Nst = N) of everybody; traj_sel [B][T][MPC_NDISC] records it
 *   7. the gather of the handle's kind at ti into the rows of the FIRING agents alone, and sel_plan[b] = sel[b] for them:
 *      a held agent's row stays the one its plan was solved on
 *   8. mpc_solve_active(fire); 9. the rate table's u_prev write; 10. the step of mpc_closed_loop_event (plant, nominal
 *      state, held, solved, solve_count, fail_count, disturbance)
 *  11. traj_clear[.][t] as in mpc_closed_loop_obstacles: the realised clearance on the new states
 * held, sel_plan, U and lambda are in/out: a second call with t0 + T and what the first returned continues both the script
 * and the holding.  U returns as last solved (not shifted by the stages applied since).  MPC_E_ARG: what
 * mpc_closed_loop_event, mpc_closed_loop_obstacles and mpc_obstacle_trigger refuse, and a NULL sel_plan. */
int mpc_rollout_held(mpc_handle *h, int B, const double *x, const double *U, const int32_t *held, double *X, void *stream);
int mpc_obstacle_trigger(mpc_handle *h, int B, int G, int K, int Lt, int wrap, int ti, const double *X, const double *obs,
                         double reach, const int32_t *held, const int32_t *sel_plan, double clear_thr, int watch,
                         const int32_t *fire_in, int32_t *sel_chk, double *clear_chk, uint8_t *why, int32_t *fire_out,
                         void *stream);
int mpc_closed_loop_obstacles_event(mpc_handle *h, int B, int T, int shift, const double *w, double thr, int max_hold, int G,
                                    int K, int Lt, int wrap, int t0, const double *obs, double reach, double clear_thr,
                                    int watch, double *x, const double *cl, int32_t *cl_index, double *U, double *lambda,
                                    int32_t *held, int32_t *sel_plan, double *table, const double *disturbance,
                                    double *traj_x, double *traj_u, int32_t *traj_sel, double *traj_clear,
                                    uint8_t *traj_why, uint8_t *solved, int32_t *solve_count, int32_t *fail_count,
                                    double *stats, void *stream, const mpc_track *trk);

/* Event-triggered holding in traffic: the car trigger watches the plant alone, and an opponent that changes its plan does
 * not move my plant off my plan; these two calls add the trigger that watches the other agents' plans.  It is time-aligned
 * by construction: mpc_rollout_held's X[b][j] is the state agent b reaches at time now + j + 1 whether b has just
 * re-planned or is held[b] stages into its plan, so one X serves the selection and the gather of the whole batch.
 * mpc_opponent_trigger: the rule of mpc_obstacle_trigger on the other agents, pure -- it shifts no plan and rewrites no
 * table.  The scene arguments (G, radius, reach) are mpc_opponents_from_plans'; X [B][N][nx] is mpc_rollout_held's; opp_plan
 * [B][MPC_NDISC] (int32) holds the GLOBAL indices of the agents the held plan was solved against (-1: none).  With k_b =
 * min(max(held[b], 0), N - 1) and n_b = N - k_b, the selection of mpc_opponents_from_plans runs for agent b over the stages
 * j < n_b and no others: c(b, o) = min_{j < n_b} g_j.  The count is b's own, not the opponent's -- o's positions are read as
 * X has them, its own repeated tail included: that is what o goes on applying as far as anyone knows, and what a gather at
 * this step copies.  A non-finite g_j at j < n_b takes the pair out, one at j >= n_b is never looked at.  opp_chk
 * [B][MPC_NDISC] (int32) and clear_chk [B][MPC_NDISC] (out; -1 and +inf for an unused slot).  Then why [B] (uint8, out,
 * NULL ok) and fire_out [B] (int32, out; may be fire_in) are mpc_obstacle_trigger's, word for word, with opp_chk for sel_chk
 * and opp_plan for sel_plan:
 *     bit 0 (1)  fire_in[b] != 0 (NULL: none)
 *     bit 1 (2)  held[b] > 0, watch & 1 and !(clear_chk[b][0] >= clear_thr)
 *     bit 2 (4)  held[b] > 0, watch & 2 and some opp_chk[b][j] >= 0 is not a member of {opp_plan[b][0], opp_plan[b][1]}
 * Asynchronous on `stream`.  MPC_E_ARG before any launch: everything mpc_opponents_from_plans refuses (Nst = N), clear_thr >
 * reach^2 or NaN, watch outside [0, 3], a NULL X, held, opp_plan, opp_chk, clear_chk or fire_out.
 * mpc_closed_loop_traffic_event: mpc_closed_loop_traffic(_field) in which an agent keeps applying the plan it holds.  The
 * arguments are those of mpc_closed_loop_event (w, thr, max_hold, held, disturbance, solved, solve_count) and of the traffic
 * loops (G, radius, reach, table, traj_opp, traj_clear), clear_thr and watch as above, opp_plan [B][MPC_NDISC] (in/out) and
 * traj_why [B][T] (uint8, NULL ok).  On a handle of MPC_CONSTR_DISCS `table` is the bound disc table and `shape` must be
 * NULL; on every other handle `table` is the bound field table and shape [B][4] is required (mpc_fields_from_plans').  The
 * table has P == B rows and so has a bound rate table, as in the traffic loops.  Blocking.  Step t, every launch being the one
 * the public call of that name makes:
 *   1. fire = mpc_trigger_eval(x, xhat, held) -- no plan is shifted yet; a handle that has no nominal states for this B
 *      fires everybody at its first step, as in mpc_closed_loop_event
 *   2. X = mpc_rollout_held(x, U, held), into a buffer of the handle
 *   3. fire, traj_why[.][t] = mpc_opponent_trigger(X, held, opp_plan, fire_in = fire)
 *   4. shift != 0: the plans of the firing agents with held > 0 are shifted in place by k_b stages
 *   5. opp = mpc_opponents_from_plans(X, Nst = N) of everybody; traj_opp [B][T][MPC_NDISC] records it
 *   6. the gather of the handle's kind (mpc_discs_from_plans / mpc_fields_from_plans) from X and opp into the rows of the
 *      FIRING agents alone, and opp_plan[b] = opp[b] for them: a held agent's row stays the one its plan was solved on
 *   7. mpc_solve_active(fire); lambda is NOT re-slotted
 *   8. the rate table's u_prev write
 *   9. the step of mpc_closed_loop_event (plant, nominal state, held, solved, solve_count, fail_count, disturbance)
 *  10. traj_clear[.][t] as in mpc_closed_loop_traffic: slot 0 of the selection on the new states (Nst = 1, reach = +inf)
 * A held agent sees an opponent's re-plan at the step after it (the X of step 2 is rolled from the plans before the solve
 * of step 7), as in a Jacobi sweep.  held, opp_plan, U and lambda are in/out: a second call with what the first returned
 * continues it.  U returns as last solved (not shifted by the stages applied since).  thr = 0 with shift != 0 is
 * mpc_closed_loop_traffic(_field) bit for bit; G = 1 is mpc_closed_loop_event on a table of zeros; watch = 0 fires by
 * deviation and hold limit alone.  MPC_E_ARG, before the first allocation: what mpc_closed_loop_event, the traffic loops and
 * mpc_opponent_trigger refuse, a NULL opp_plan, a shape on a disc handle and none on another. */
int mpc_opponent_trigger(mpc_handle *h, int B, int G, const double *X, const double *radius, double reach,
                         const int32_t *held, const int32_t *opp_plan, double clear_thr, int watch,
                         const int32_t *fire_in, int32_t *opp_chk, double *clear_chk, uint8_t *why,
                         int32_t *fire_out, void *stream);
int mpc_closed_loop_traffic_event(mpc_handle *h, int B, int T, int shift, const double *w, double thr, int max_hold,
                                  int G, const double *radius, const double *shape, double reach, double clear_thr, int watch,
                                  double *x, const double *cl, const int32_t *cl_index, double *U, double *lambda,
                                  int32_t *held, int32_t *opp_plan, double *table, const double *disturbance,
                                  double *traj_x, double *traj_u, int32_t *traj_opp, double *traj_clear, uint8_t *traj_why,
                                  uint8_t *solved, int32_t *solve_count, int32_t *fail_count, double *stats, void *stream);

/* profiling aid: rounds (eval launches) and kernel time of the last mpc_solve_batch */
int mpc_last_solve_info(mpc_handle *h, int64_t *rounds, int64_t *evals_grad, int64_t *evals_cost,
                        double *eval_ms, double *step_ms);
/* f-3 (game_theory.py:115-244 Car.get_total_payoff and its parts): lane-change payoffs of B traffic
 * scenes.  params15 (HOST array) = [L, W, l, theta_max, tlc, td, ti, tau, a_max, h, Lf, q1, q2, a, b]
 * (game_theory.py:23-40,:115,:205); ego [B][3] = (x, v, lane); cars [B][K][3]; ncars [B] <= K <= 62;
 * out [B][2][4] = target lane 1, 2 -> [total, safety, velocity, comfort]. */
int mpc_lane_payoff(mpc_handle *h, int B, int K, const double *params15, const double *ego,
                    const double *cars, const int32_t *ncars, double *out, void *stream);

/* test aid: evaluates the device math used by the kernels; op 0 sin, 1 cos, 2 atan, 3 atan2(a,b),
 * 4 tan, 5 exp (the out-of-line one the risk field calls) on n values */
int mpc_math_probe(mpc_handle *h, int n, int op, const double *a, const double *b, double *out,
                   void *stream);
/* more figures of the last solve: launch pairs (step, eval) issued over all sub-batch groups and
 * L-BFGS history pairs read by K3 */
int mpc_last_solve_info2(mpc_handle *h, double *launch_pairs, int64_t *lbfgs_rows);
/* speculation of the last solve: gradients evaluated ahead of need on the second channel (the
 * next iteration's Hessian-vector point, assuming the line-search trial is accepted) and how many of
 * them the next iteration consumed */
int mpc_last_speculation(mpc_handle *h, int64_t *issued, int64_t *used);
/* lookahead of the persistent kernel (Pacejka model, N <= 16, no constraints; environment MPC_NO_LOOKAHEAD at
 * mpc_create turns it off; results do not depend on it): evaluations of points the state machine was GOING to ask
 * for (next line-search trial points, deeper descent-lemma levels) executed in idle lanes beside a requested
 * evaluation, and requests later served from them without an evaluation trip */
int mpc_last_lookahead(mpc_handle *h, int64_t *evals, int64_t *hits);
/* profile mode: summed HIP-event durations (ms) of the last solve's kernels,
 * out4 = [step_kernel, rollout_kernel (K1a), stage_kernel (K1b), adjoint_kernel (K1c)] */
int mpc_last_kernel_ms(mpc_handle *h, double *out4);
/* the same with the persistent kernel and the launch counts: ms5 / launches5 = [step_kernel, K1a rollout
 * (either kernel), K1b stage (or fused K1b+K1c), K1c adjoint (unfused launches only), solo_kernel];
 * solo_agents = agents that finished in the persistent wave-per-agent kernel.  Any pointer may be NULL. */
int mpc_last_kernel_profile(mpc_handle *h, double *ms5, int64_t *launches5, int64_t *solo_agents);
/* profile mode: persistent-kernel time of the last solve -- summed over the sub-batch groups (their launches
 * overlap in time: the sum can exceed the solve) and the longest single launch (the tail a blocking solve waits for) */
int mpc_last_solo_ms(mpc_handle *h, double *sum_ms, double *longest_ms);
/* A sub-batch group whose round holds at most `max_requests` evaluation requests leaves the rounds
 * and finishes in the persistent wave-per-agent kernel, and a batch of at most `max_requests` agents runs in
 * it from the start (0 = rounds only).  Defaults (measured): switch at 1024 requests (kinematic
 * model) / 128 (Pacejka model, whose persistent-kernel waves take a whole SIMD each); whole
 * batches up to 4096 agents (kinematic, N <= 32) / 1024 (otherwise); environment
 * MPC_SOLO_MAX (both) and MPC_SOLO_ALL (the batch bound alone).  Results do not depend on it. */
int mpc_set_solo_max(mpc_handle *h, int max_requests);
/* Two more per-launch kernel choosers, environment only (read at mpc_create; results do not depend on them):
 *   MPC_PAC_QUAD_MAX  Pacejka model: requests bound of a round up to which K1a runs four lanes per request
 *                     (rollout_quad_kernel); above it one thread per request (default 24576: the four-lane kernel
 *                     shortens a lone wave's chain, the thread kernel executes 2.2x fewer instructions).
 *   MPC_CHAIN_MIN     requests bound of a group's round from which the step launch carries the thread-per-agent
 *                     blocks that serve agents waiting for a trial point's gradient (default 24576: full rounds of
 *                     groups of more than 12288 agents; kinematic model only unless this variable is set);
 *                     MPC_NO_CHAIN = never. */
/* sub-batch pipelining: the batch is split into `groups` contiguous ranges whose rounds run on
 * separate HIP streams (0 = automatic: 4 from 49152 agents when the runtime runs five streams side by
 * side -- measured at mpc_create, see mpc_stream_concurrency --, 3 from 24576, 2 from 16384, else 1; at
 * most 8; never fewer than 1024 agents per group).  Results do not depend on it. */
int mpc_set_groups(mpc_handle *h, int groups);
/* streams = how many of this process's streams the HIP runtime runs side by side, as far as the solver
 * cares: 5 (five or more) or 4 (fewer).  Measured when the handle is created (an idling kernel on the null
 * stream and on four streams of the handle), NOT read from GPU_MAX_HW_QUEUES: the runtime reads that
 * variable once, when it initialises, and 4 is its default -- a C caller that wants four groups exports
 * GPU_MAX_HW_QUEUES >= 5 before its first HIP call (the Python package does so at import).
 * groups_last = sub-batch groups of the last solve.  Either pointer may be NULL. */
int mpc_stream_concurrency(mpc_handle *h, int *streams, int *groups_last);
/* on != 0 (default): a failed inner solve that the outer loop backtracks over without constraints is
 * replayed from a memo -- same outcome, same counted statistics, no evaluations executed -- instead of
 * being recomputed; 0 (or the environment MPC_NO_MEMO at mpc_create): recomputed, as the reference walks.
 * Controls, multipliers and all MPC_NSTATS statistics are bit-identical either way. */
int mpc_set_memo(mpc_handle *h, int on);
/* test aid: at most `rounds` rounds (persistent kernel: evaluations per agent) per solve; a solve that
 * needs more returns MPC_E_LIMIT with the agents it could not finish left as they are (0 = the built-in
 * guard alone, which no valid solve reaches) */
int mpc_set_round_limit(mpc_handle *h, int64_t rounds);
/* Wall-clock bound of a solve's host side (default 300 s; environment MPC_POLL_TIMEOUT_S at mpc_create).  The
 * round loop of mpc_solve_batch is host code that polls device counters: when NO polled window has completed
 * for `seconds`, or one of the blocking waits behind the loop has lasted that long, the call returns MPC_E_HIP
 * ("wall-clock bound ... expired") instead of waiting for ever on a device that does not answer.  It does NOT
 * synchronise the device on that path (that would be the same hang): kernels of the solve may still be queued and
 * the caller's U / lambda / stats buffers are in use until the caller has synchronised the device itself.  A
 * valid solve never comes near the default (a 65 536-agent solve completes a window every ~3 ms). */
int mpc_set_poll_timeout(mpc_handle *h, double seconds);
/* test aid: queues the library's idling kernel (one wavefront sleeping for `microseconds` of the device wall
 * clock, at most 30 s) on `stream` */
int mpc_debug_spin(mpc_handle *h, double microseconds, void *stream);
/* diagnostic: the per-agent solver records as the last solve left them, decoded to plain doubles, copied to the
 * HOST array host_out [B][MPC_NREC] (B <= the last solve's batch); mpc_debug_record_names() = the comma-separated
 * names of the slots in use (step sizes L / gamma, accepted line-search step tau (halved), |J|, history fill,
 * evaluation counters ...).  After a solve stopped by max_total_inner = k the records hold the solver state after
 * k inner iterations: what tests/test_gpu_parity.py::test_iterate_prefix_parity and tools/dev/first_divergence.py
 * compare with the oracle's per-iteration trace.  Synchronises the device. */
int mpc_debug_records(mpc_handle *h, int B, double *host_out);
const char *mpc_debug_record_names(void);
/* on != 0: bracket every kernel of mpc_solve_batch with HIP events on the solve's stream so that
 * mpc_last_solve_info reports eval_ms / step_ms (also enabled by the environment MPC_PROFILE=1) */
int mpc_set_profile(mpc_handle *h, int on);

#ifdef __cplusplus
}
#endif
#endif
