// mpc_api.hip -- the C-ABI of libmpc_hip.so (see include/mpc_hip.h): the extern "C" entry points of the batched MPC
// solve on one MI355X, one process / one handle per GPU.  The one translation unit of the library: the host side is in
// mpc_handle.hpp (the handle and its per-agent tables), mpc_launch.hpp (which kernel instantiation a launch takes) and mpc_rounds.hpp (the
// round loop of a solve), the kernels in the headers those include (and mpc_track.hpp: the kernels of lap driving;
// mpc_obstacles.hpp: the kernels of the scripted obstacles).
#include "mpc_rounds.hpp"
#include "mpc_track.hpp"
#include "mpc_obstacles.hpp"

extern "C" const char *mpc_last_error(void) { return g_err.c_str(); }
#ifndef MPC_SOURCE_SHA256
#define MPC_SOURCE_SHA256 "unknown"
#endif
extern "C" const char *mpc_source_hash(void) { return MPC_SOURCE_SHA256; }

extern "C" int mpc_default_config(mpc_config *c, int model, int N)
{
    if (!c || N < 1 || N > MPC_MAX_N || (model != MPC_MODEL_KINEMATIC && model != MPC_MODEL_PACEJKA))
        return fail(MPC_E_ARG, "mpc_default_config: bad model or horizon");
    std::memset(c, 0, sizeof(*c));
    c->model = model; c->N = N;
    c->S = 100;            // main.py:70
    c->nfe = 4;            // car_dynamics.py:136
    c->wrap_mode = MPC_WRAP_FLOOR;
    c->lbfgs_memory = N;   // controller.py:36
    c->max_iter = 1000;    // controller.py:31
    c->max_outer = 1000;   // controller.py:45
    c->hess_heuristic = 15; // controller.py:32
    c->max_no_progress = 10;
    c->Ts = 0.05;          // car_dynamics.py:93
    c->v_ref = 1.0;        // main.py:65
    const double w[6] = {0.5, 1.0, 1.0, 0.5, 0.1, 0.01}; // car_dynamics.py:230
    std::memcpy(c->cost_w, w, sizeof w);
    const double veh[22] = {9.7e-2, 4.7e-2, 5e-2, 0.09, 0.07, 8e-2, 5.5e-2, 0.1735, 18.3e-5, // main.py:84
                            0.32, 1.0,                                                      // main.py:82
                            0.268, 2.165, 3.47, 0.242, 2.38, 2.84,                          // main.py:85
                            0.266, 0.1, 0.1025, 0.1629, 0.0011};                            // main.py:86
    std::memcpy(c->veh, veh, sizeof veh);
    c->accel = 2.0; c->friction = 1.0; // dynamics.py:34-35
    c->u_lb[0] = -1.0; c->u_ub[0] = 1.0; c->u_lb[1] = -0.32; c->u_ub[1] = 0.32; // main.py:55-56
    const double off[6] = {20, 1, 1, 2, 1, 0.1}; // main.py:46-51
    std::memcpy(c->g_off, off, sizeof off);
    for (int i = 0; i < 6; i++) { c->D_lb[i] = -INFINITY; c->D_ub[i] = INFINITY; }
    c->lane_halfwidth = 0.15;
    c->alm_eps = 1e-6; c->alm_delta = 1e-4; c->Sigma0 = 1e5; // controller.py:41-43
    c->eps0 = 1.0; c->rho = 0.1; c->Delta = 10.0; c->theta = 0.1; c->M = 1e9; c->Sigma_max = 1e9;
    c->Delta_lower = 0.8; c->Sigma0_lower = 0.6; c->eps0_increase = 1.1; c->rho_increase = 2.0;
    c->max_num_initial_retries = 20; c->max_num_retries = 20; c->max_total_num_retries = 40;
    c->max_total_inner = 5000; c->max_total_evals = 0;
    c->lip_eps = 1e-6; c->lip_delta = 1e-12; c->Lgamma_factor = 0.95;
    c->L_min = 1e-5; c->L_max = 1e20; c->tau_min = 1.0 / 256; c->qub_tol = 10 * DBL_EPSILON;
    return MPC_OK;
}

extern "C" int mpc_nx(const mpc_config *c) { return c->model == MPC_MODEL_PACEJKA ? 6 : 4; }
extern "C" int mpc_m(const mpc_config *c) { return stage_m(c) * c->N; }

static_assert(MPC_NPARAM == mpc::NPARAM, "row layout: include/mpc_hip.h and mpc_device.hpp");
extern "C" int mpc_default_params(const mpc_config *c, double *row)
{
    if (!c || !row) return fail(MPC_E_ARG, "mpc_default_params: null argument");
    for (int i = 0; i < 22; i++) row[i] = c->veh[i];
    row[22] = c->accel; row[23] = c->friction; row[24] = c->v_ref;
    for (int i = 0; i < 6; i++) row[25 + i] = c->cost_w[i];
    return MPC_OK;
}

static_assert(MPC_NBOUND == mpc::NBOUND, "row layout: include/mpc_hip.h and mpc_device.hpp");
extern "C" int mpc_default_bounds(const mpc_config *c, double *row)
{
    if (!c || !row) return fail(MPC_E_ARG, "mpc_default_bounds: null argument");
    row[0] = c->u_lb[0]; row[1] = c->u_lb[1]; row[2] = c->u_ub[0]; row[3] = c->u_ub[1];
    return MPC_OK;
}

static_assert(MPC_NCONSTR == mpc::NCONSTR, "row layout: include/mpc_hip.h and mpc_device.hpp");
extern "C" int mpc_default_constraints(const mpc_config *c, double *row)
{
    if (!c || !row) return fail(MPC_E_ARG, "mpc_default_constraints: null argument");
    for (int i = 0; i < 6; i++) { row[i] = c->g_off[i]; row[6 + i] = c->D_lb[i]; row[12 + i] = c->D_ub[i]; }
    row[18] = c->lane_halfwidth;
    return MPC_OK;
}

static_assert(MPC_NDISC == mpc::NDISC, "row layout: include/mpc_hip.h and mpc_device.hpp");
extern "C" int mpc_default_discs(const mpc_config *c, double *row)
{
    if (!c || !row) return fail(MPC_E_ARG, "mpc_default_discs: null argument");
    if (c->N < 1 || c->N > MPC_MAX_N) return fail(MPC_E_ARG, "mpc_default_discs: horizon N out of range [1, 64]");
    for (int i = 0; i < MPC_DISC_ROW(c->N); i++) row[i] = 0.0;   // r = 0: no obstacle at any stage
    return MPC_OK;
}

static_assert(MPC_NRATE == mpc::NRATE, "row layout: include/mpc_hip.h and mpc_device.hpp");
extern "C" int mpc_default_rates(const mpc_config *c, double *row)
{
    if (!c || !row) return fail(MPC_E_ARG, "mpc_default_rates: null argument");
    for (int i = 0; i < MPC_NRATE; i++) row[i] = 0.0;   // no move penalty, u_{-1} = 0
    return MPC_OK;
}

static_assert(MPC_NFIELD == mpc::NFIELD && MPC_NFSRC == mpc::NFSRC, "row layout: include/mpc_hip.h and mpc_device.hpp");
static_assert(MPC_NFIELD == MPC_NDISC, "one opp [B][2] of mpc_opponents_from_plans serves the discs and the fields");
extern "C" int mpc_default_fields(const mpc_config *c, double *row)
{
    if (!c || !row) return fail(MPC_E_ARG, "mpc_default_fields: null argument");
    if (c->N < 1 || c->N > MPC_MAX_N) return fail(MPC_E_ARG, "mpc_default_fields: horizon N out of range [1, 64]");
    for (int i = 0; i < MPC_FIELD_ROW(c->N); i++) row[i] = 0.0;   // A = 0: no obstacle at any stage
    return MPC_OK;
}

static_assert(MPC_NROAD == mpc::NROAD, "row layout: include/mpc_hip.h and mpc_device.hpp");
extern "C" int mpc_default_roads(const mpc_config *c, double *row)
{
    if (!c || !row) return fail(MPC_E_ARG, "mpc_default_roads: null argument");
    if (c->N < 1 || c->N > MPC_MAX_N) return fail(MPC_E_ARG, "mpc_default_roads: horizon N out of range [1, 64]");
    for (int i = 0; i < MPC_ROAD_ROW(c->N); i++) row[i] = 0.0;   // every weight 0: no part is on at any stage
    return MPC_OK;
}

extern "C" int mpc_create(const mpc_config *cfg, int device, mpc_handle **out)
{
    if (!cfg || !out) return fail(MPC_E_ARG, "mpc_create: null argument");
    {   // the configuration is checked before anything touches the device (and without one: CPU tests)
        DevCfg probe;
        const int rcv = make_devcfg(*cfg, probe);
        if (rcv) return rcv;
    }
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(MPC_E_ARG, "mpc_create: no such device");
    mpc_handle *h = new mpc_handle();
    // Pacejka model: 128.  Its persistent-kernel waves take a whole SIMD each (512 registers); the 2 237 agents that four
    // groups hand over at 1 024 requests each are more than the chip's 1 024 SIMDs hold, the later groups' waves queue and
    // the ones in flight starve the other groups' rounds, while a thin Pacejka round is no slower per evaluation than a
    // lone wave's trip (round 4, same box, alternating, 65 536 agents, bit-identical: 1 024 -> 462 ms, 512 -> 447,
    // 384 -> 426, 32 .. 256 -> 412 - 429).  Kinematic model: 1 024 as measured in round 2 (its trips are 4x shorter than
    // a thin round, two waves per SIMD).
    h->solo_max = cfg->model == MPC_MODEL_PACEJKA ? 128 : 1024;
    h->solo_all = (cfg->model == MPC_MODEL_KINEMATIC && cfg->N <= 32) ? 4096 : 1024;
    h->cfg = *cfg;
    int rc = make_devcfg(*cfg, h->dc);
    if (rc) { delete h; return rc; }
    h->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) h->num_cus = cus;
    }
    if (e == hipSuccess) e = h->pinned_mem.alloc(sizeof(PinnedCounts));
    if (e != hipSuccess) { delete h; return fail(MPC_E_HIP, std::string("mpc_create: ") + hipGetErrorString(e)); }
    read_switches(h);
    *out = h;
    return MPC_OK;
}

extern "C" int mpc_destroy(mpc_handle *h)
{
    if (!h) return MPC_OK;
    if (h->worker.joinable()) {           // a solve still running finishes first
        { std::lock_guard<std::mutex> lk(h->mu); h->worker_quit = true; }
        h->cv.notify_all();
        h->worker.join();
    }
    (void)hipSetDevice(h->device);
    if (h->syncev) (void)hipEventDestroy(h->syncev);
    for (auto ev : h->ev_pool) (void)hipEventDestroy(ev);
    for (int g = 0; g < MPC_MAX_GROUPS; g++) if (h->gstream[g]) (void)hipStreamDestroy(h->gstream[g]);
    for (int g = 0; g <= MPC_MAX_GROUPS; g++) if (h->gevent[g]) (void)hipEventDestroy(h->gevent[g]);
    for (int b = 0; b < 2; b++) for (int g = 0; g < MPC_MAX_GROUPS; g++) if (h->pollev[b][g]) (void)hipEventDestroy(h->pollev[b][g]);
    for (int b = 0; b < 2; b++) for (int g = 0; g < MPC_MAX_GROUPS; g++) if (h->soloev[g][b]) (void)hipEventDestroy(h->soloev[g][b]);
    delete h;   // (and with it every DevBuf: the handle's memory)
    return MPC_OK;
}

extern "C" int mpc_centerline_blocks(mpc_handle *h, const double *cl, int C, void *stream)
{
    int rc = check_common(h, C, "mpc_centerline_blocks"); if (rc) return rc;
    h->cl_grid_for = nullptr;
    // the grid costs 256 KB per centerline row: a table with one row per agent keeps the full scan
    if (C == 0 || !cl || C > MPC_GRID_MAX_ROWS) return MPC_OK;
    const DevCfg &c = h->dc;
    GridBufs &g = h->grid;
    if (C > g.cap) {   // (not zero-filled: the two kernels write all of it)
        g.cap = 0;
        rc = carve(g.arena, h->device, false, "centerline grid hipMalloc failed", [&](Carver &a) { grid_layout(a, g, (size_t)c.S, (size_t)C); });
        if (rc) return rc;
        g.cap = C;
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cl_grid_meta_kernel, dim3((unsigned)C), dim3(64), 0, s, c, cl, C, g.gmeta, g.gxy);
    hipLaunchKernelGGL(cl_grid_cells_kernel, dim3(GRID_CELLS / 256, C), dim3(256), 0, s, c, cl, C, g.gmeta, g.gcells);
    HIPCHK(hipGetLastError());
    h->cl_grid_for = cl;
    return MPC_OK;
}

// What a row of each kind must satisfy to be bound (`where`: "<setter>: row <p>", the head of the refusal) -- the one
// real difference between the three setters.
// parameters: what the model divides by must be positive and everything finite
static int param_row_rule(const mpc_handle *h, const double *r, const std::string &where)
{
    for (int i = 0; i < MPC_NPARAM; i++)
        if (!std::isfinite(r[i])) return fail(MPC_E_ARG, where + ", value " + std::to_string(i) + " is not finite");
    if (!(r[1] + r[2] > 0.0)) return fail(MPC_E_ARG, where + ": lf + lr (veh[1] + veh[2]) must be positive");
    if (h->cfg.model == MPC_MODEL_PACEJKA && (!(r[7] > 0.0) || !(r[8] > 0.0)))
        return fail(MPC_E_ARG, where + ": mass and inertia (veh[7], veh[8]) must be positive");
    return MPC_OK;
}
// input boxes: the rule mpc_create applies to the handle's box
static int box_row_rule(const mpc_handle *, const double *r, const std::string &where)
{
    return box_ok(r, r + 2) ? MPC_OK : fail(MPC_E_ARG, where + ": u_lb must not exceed u_ub");
}
// constraint data: the fields the handle's constr_mode reads
static int constr_row_rule(const mpc_handle *h, const double *r, const std::string &where)
{
    if (h->cfg.constr_mode == MPC_CONSTR_LANE)
        return std::isfinite(r[18]) && r[18] > 0.0 ? MPC_OK : fail(MPC_E_ARG, where + ": lane_halfwidth must be finite and positive");
    for (int i = 0; i < mpc_nx(&h->cfg); i++) {
        if (!std::isfinite(r[i])) return fail(MPC_E_ARG, where + ": g_off[" + std::to_string(i) + "] is not finite");
        if (!(r[6 + i] <= r[12 + i])) return fail(MPC_E_ARG, where + ": D_lb must not exceed D_ub");
    }
    return MPC_OK;
}

// keep-out discs: every value finite, no negative radius
static int disc_row_rule(const mpc_handle *h, const double *r, const std::string &where)
{
    for (int i = 0; i < h->cfg.N * MPC_NDISC; i++) {
        const std::string which = ", stage " + std::to_string(i / MPC_NDISC) + ", disc " + std::to_string(i % MPC_NDISC);
        for (int f = 0; f < 3; f++)
            if (!std::isfinite(r[3 * i + f])) return fail(MPC_E_ARG, where + which + ": (cx, cy, r) must be finite");
        if (!(r[3 * i + 2] >= 0.0)) return fail(MPC_E_ARG, where + which + ": the radius must not be negative");
    }
    return MPC_OK;
}

// move penalties: everything finite, no negative weight
static int rate_row_rule(const mpc_handle *, const double *r, const std::string &where)
{
    for (int i = 0; i < MPC_NRATE; i++)
        if (!std::isfinite(r[i])) return fail(MPC_E_ARG, where + ": (w_d, w_delta, d_prev, delta_prev) must be finite");
    if (!(r[0] >= 0.0) || !(r[1] >= 0.0)) return fail(MPC_E_ARG, where + ": the weights must not be negative");
    return MPC_OK;
}

// risk fields: every value finite, no negative height or width coefficient, and a skew only where the Gaussian along the
// frame bounds it (alpha != 0 with kx = 0 would make E = alpha a unbounded below)
static int field_row_rule(const mpc_handle *h, const double *r, const std::string &where)
{
    for (int i = 0; i < h->cfg.N * MPC_NFIELD; i++) {
        const double *q = r + (size_t)MPC_NFSRC * i;
        const std::string which = ", stage " + std::to_string(i / MPC_NFIELD) + ", source " + std::to_string(i % MPC_NFIELD);
        for (int f = 0; f < MPC_NFSRC; f++)
            if (!std::isfinite(q[f])) return fail(MPC_E_ARG, where + which + ": (cx, cy, c, s, A, kx, ky, alpha) must be finite");
        if (!(q[4] >= 0.0) || !(q[5] >= 0.0) || !(q[6] >= 0.0)) return fail(MPC_E_ARG, where + which + ": A, kx and ky must not be negative");
        if (q[7] != 0.0 && !(q[5] > 0.0)) return fail(MPC_E_ARG, where + which + ": a skew (alpha != 0) needs kx > 0");
    }
    return MPC_OK;
}

// road data: every value finite, no negative weight, and the two edges in order where both are on
static int road_row_rule(const mpc_handle *h, const double *r, const std::string &where)
{
    for (int k = 0; k < h->cfg.N; k++) {
        const double *q = r + (size_t)MPC_NROAD * k;
        const std::string which = ", stage " + std::to_string(k);
        for (int f = 0; f < MPC_NROAD; f++)
            if (!std::isfinite(q[f])) return fail(MPC_E_ARG, where + which + ": (off, w_off, lo, w_lo, hi, w_hi, v_tgt, w_v) must be finite");
        if (!(q[1] >= 0.0) || !(q[3] >= 0.0) || !(q[5] >= 0.0) || !(q[7] >= 0.0))
            return fail(MPC_E_ARG, where + which + ": the weights must not be negative");
        if (q[3] != 0.0 && q[5] != 0.0 && q[2] > q[4]) return fail(MPC_E_ARG, where + which + ": lo must not exceed hi where both edges are on");
    }
    return MPC_OK;
}

// Binds (table != NULL) or unbinds the per-agent table of one kind.  The rows are checked once, here, through a
// synchronous copy (binding is not on the hot path; rows rewritten in place later are the caller's to keep valid).
// Nothing else is done: the kernels read the caller's memory at every call.  The box and constraint forms of some
// kernels exist beside the parameter (and box) form alone: binding either makes the handle's own one-row tables.
static int bind_agent_table(mpc_handle *h, TableKind kind, const double *table, int P, const int32_t *index, int B,
                            int (*row_rule)(const mpc_handle *, const double *, const std::string &))
{
    const char *who = k_tables[kind].setter;
    { const int rb = refuse_if_busy(h, who); if (rb) return rb; }
    const size_t width = h->table_width(kind);
    if (!table) { h->tab[kind] = BoundTable{}; return MPC_OK; }
    if (kind == TAB_CONSTR && h->cfg.constr_mode == MPC_CONSTR_NONE)
        return fail(MPC_E_ARG, std::string(who) + ": the handle has no general constraints (constr_mode MPC_CONSTR_NONE)");
    if (kind == TAB_CONSTR && h->cfg.constr_mode == MPC_CONSTR_DISCS)
        return fail(MPC_E_ARG, std::string(who) + ": the handle's constraints are keep-out discs (constr_mode MPC_CONSTR_DISCS): "
                                                  "there is no constraint data to bind (mpc_set_agent_discs)");
    if (kind == TAB_DISCS && h->cfg.constr_mode != MPC_CONSTR_DISCS)
        return fail(MPC_E_ARG, std::string(who) + ": the handle's constr_mode is not MPC_CONSTR_DISCS");
    if (kind == TAB_FIELDS && h->cfg.constr_mode == MPC_CONSTR_DISCS)
        return fail(MPC_E_ARG, std::string(who) + ": the handle's constraints are keep-out discs (constr_mode MPC_CONSTR_DISCS): there an "
                                                  "obstacle is a disc (mpc_set_agent_discs)");
    // A field, road or rate table together with a constraint table would need kernel forms that take both (with_table_form
    // in mpc_launch.hpp has none): whichever comes second is refused, a constraint table for the first of the three in this order
    for (const TableKind x : {TAB_FIELDS, TAB_ROADS, TAB_RATES}) {
        const TableKind other = kind == x ? TAB_CONSTR : x;
        if ((kind == x || kind == TAB_CONSTR) && h->tab[other].table)
            return fail(MPC_E_ARG, std::string(who) + ": a " + k_tables[other].noun + " table is bound (" + k_tables[other].setter +
                                   "): a " + k_tables[x].noun + " table and a constraint table cannot be bound together");
    }
    if (P < 1 || B < 1 || !index) return fail(MPC_E_ARG, std::string(who) + ": need P >= 1 rows, B >= 1 agents and an index");
    { const int ra = check_tables_agree(h, B, who, kind); if (ra) return ra; }
    HIPCHK(hipSetDevice(h->device));
    std::vector<double> rows((size_t)P * width);
    HIPCHK(hipMemcpy(rows.data(), table, rows.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int p = 0; p < P; p++) {
        const int rr = row_rule(h, rows.data() + (size_t)p * width, std::string(who) + ": row " + std::to_string(p));
        if (rr) return rr;
    }
    if (kind != TAB_PARAMS) { const int ro = reserve_own_tables(h, B, who); if (ro) return ro; }
    h->tab[kind] = BoundTable{table, index, P, B};
    return MPC_OK;
}

extern "C" int mpc_set_agent_params(mpc_handle *h, const double *table, int P, const int32_t *index,
                                    const int32_t *plant_index, int B)
{
    const int rc = bind_agent_table(h, TAB_PARAMS, table, P, index, B, param_row_rule);
    if (rc == MPC_OK) h->pidx_plant = table ? plant_index : nullptr;
    return rc;
}
extern "C" int mpc_set_agent_bounds(mpc_handle *h, const double *table, int P, const int32_t *index, int B)
{
    return bind_agent_table(h, TAB_BOX, table, P, index, B, box_row_rule);
}
extern "C" int mpc_set_agent_constraints(mpc_handle *h, const double *table, int P, const int32_t *index, int B)
{
    return bind_agent_table(h, TAB_CONSTR, table, P, index, B, constr_row_rule);
}

extern "C" int mpc_set_agent_discs(mpc_handle *h, const double *table, int P, const int32_t *index, int B)
{
    return bind_agent_table(h, TAB_DISCS, table, P, index, B, disc_row_rule);
}

extern "C" int mpc_set_agent_rates(mpc_handle *h, const double *table, int P, const int32_t *index, int B)
{
    return bind_agent_table(h, TAB_RATES, table, P, index, B, rate_row_rule);
}
extern "C" int mpc_set_agent_fields(mpc_handle *h, const double *table, int P, const int32_t *index, int B)
{
    return bind_agent_table(h, TAB_FIELDS, table, P, index, B, field_row_rule);
}
extern "C" int mpc_set_agent_roads(mpc_handle *h, const double *table, int P, const int32_t *index, int B)
{
    return bind_agent_table(h, TAB_ROADS, table, P, index, B, road_row_rule);
}
// The closed loops carry u_{-1} themselves: with a rate table bound they need a row per agent (P == B; index 0 .. B-1 is
// the caller's to ensure, as with the traffic loop's disc table) ...
static int check_rate_rows(const mpc_handle *h, int B, const std::string &who)
{
    const BoundTable &rt = h->tab[TAB_RATES];
    if (rt.table && rt.rows != B)
        return fail(MPC_E_ARG, who + ": the bound rate table has " + std::to_string(rt.rows) + " rows, the loop writes the applied input into "
                               "one per agent (P == B = " + std::to_string(B) + ", index 0 .. B-1)");
    return MPC_OK;
}
// ... and write the input about to be applied into it, behind the solve and before the plant moves (rate_prev_kernel)
static void launch_rate_prev(mpc_handle *h, hipStream_t s, int B, const double *U, const int32_t *held, const int32_t *fire)
{
    const BoundTable &rt = h->tab[TAB_RATES];
    if (rt.table)
        hipLaunchKernelGGL(rate_prev_kernel, grid_for(B, 64), dim3(64), 0, s, B, h->cfg.N, U, held, fire, const_cast<double *>(rt.table), rt.idx);
}

// What the loops that rewrite a per-agent table in place (the traffic loops, the obstacle loop) ask of it: `table` is the
// bound table of `kind`, with a row per agent
static int check_rewritten_table(const mpc_handle *h, TableKind kind, const double *table, int B, const std::string &who)
{
    const BoundTable &dt = h->tab[kind];
    if (!table || table != dt.table)
        return fail(MPC_E_ARG, who + ": table must be the " + k_tables[kind].noun + " table that is bound (" + k_tables[kind].setter +
                               "): the loop rewrites it in place");
    if (dt.rows != B)
        return fail(MPC_E_ARG, who + ": the bound " + k_tables[kind].noun + " table has " + std::to_string(dt.rows) +
                               " rows, the loop needs one per agent (P == B = " + std::to_string(B) + ", index 0 .. B-1)");
    return MPC_OK;
}
// The body of every closed loop whose step ends in plant_step_kernel: T times before(t), the solve, u_{-1} into the rate
// table, the plant step, after(t) -- before and after launch what the loop does around a step and return an rc -- then
// the check for a failed launch.  The final wait is the caller's.  (The event-triggered loops have another step.)
template <class Before, class After>
static int plant_loop(mpc_handle *h, int B, int T, int shift, double *x, const double *cl, const int32_t *cl_index, double *U,
                      double *lambda, double *traj_x, double *traj_u, int32_t *fail_count, double *stats, void *stream, Before before,
                      After after)
{
    // the solves' statistics: into the caller's buffer, or the handle's stage buffer
    int rc = stats ? MPC_OK : reserve_stage(h, sizeof(double) * 8 * (size_t)B); if (rc) return rc;
    double *st = stats ? stats : (double *)h->stage.p;
    hipStream_t s = (hipStream_t)stream;
    for (int t = 0; t < T; t++) {
        rc = before(t); if (rc) return rc;
        rc = mpc_solve_batch(h, B, x, cl, cl_index, U, lambda, st, stream); if (rc) return rc;
        launch_rate_prev(h, s, B, U, nullptr, nullptr);
        // bound parameter table: the controller solves with row pidx[b], the plant advances with row pidx_plant[b] (null: the same)
        with_model_table(h, h->plant_rows(), [&](auto MODEL, auto PA, auto... pt) {
            hipLaunchKernelGGL((plant_step_kernel<MODEL(), PA(), decltype(pt)...>), grid_for(B, 64), dim3(64), 0,
                               s, h->dc, B, t, T, shift, x, U, traj_x, traj_u, st, fail_count, pt...);
        });
        rc = after(t); if (rc) return rc;
    }
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

// What the two public gathers from plans share (`kernel`: discs_from_plans_kernel with `per` = radius [B], or
// fields_from_plans_kernel with `per` = shape [B][4]): a pure gather, asynchronous
template <class Kernel>
static int rows_from_plans(const std::string &who, Kernel kernel, mpc_handle *h, int B, const double *X, const int32_t *opp,
                           const double *per, double *table, void *stream)
{
    int rc = check_common(h, B, who.c_str()); if (rc) return rc;
    if (B == 0) return MPC_OK;
    if (!X || !opp || !per || !table) return fail(MPC_E_ARG, who + ": null buffer");
    const size_t words = (size_t)B * h->cfg.N * MPC_NDISC;   // (== MPC_NFIELD)
    hipLaunchKernelGGL(kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B, h->cfg.N, h->dc.nx, X, opp,
                       per, table);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}
extern "C" int mpc_discs_from_plans(mpc_handle *h, int B, const double *X, const int32_t *opp, const double *radius,
                                    double *table, void *stream)
{
    return rows_from_plans("mpc_discs_from_plans", discs_from_plans_kernel<>, h, B, X, opp, radius, table, stream);
}
extern "C" int mpc_fields_from_plans(mpc_handle *h, int B, const double *X, const int32_t *opp, const double *shape,
                                     double *table, void *stream)
{
    return rows_from_plans("mpc_fields_from_plans", fields_from_plans_kernel<>, h, B, X, opp, shape, table, stream);
}

extern "C" int mpc_rhs(mpc_handle *h, int B, const double *x, const double *u, double *dx, void *stream)
{
    int rc = check_common(h, B, "mpc_rhs"); if (rc) return rc;
    if (B == 0) return MPC_OK;
    if (!x || !u || !dx) return fail(MPC_E_ARG, "mpc_rhs: null buffer");
    rc = check_tables(h, B, "mpc_rhs", READS_PARAMS); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    with_model_table(h, h->params().idx, [&](auto MODEL, auto PA, auto... pt) {
        hipLaunchKernelGGL((rhs_kernel<MODEL(), PA(), decltype(pt)...>), grid_for(B, 64), dim3(64), 0, s, h->dc, B, x, u, dx, pt...);
    });
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

extern "C" int mpc_rollout(mpc_handle *h, int B, int Nsim, const double *x0, const double *U, double *X,
                           void *stream)
{
    int rc = check_common(h, B, "mpc_rollout"); if (rc) return rc;
    if (B == 0 || Nsim == 0) return MPC_OK;
    if (Nsim < 0 || !x0 || !U || !X) return fail(MPC_E_ARG, "mpc_rollout: bad argument");
    rc = check_tables(h, B, "mpc_rollout", READS_PARAMS); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    with_model_table(h, h->params().idx, [&](auto MODEL, auto PA, auto... pt) {
        hipLaunchKernelGGL((simulate_kernel<MODEL(), PA(), decltype(pt)...>), grid_for(B, 64), dim3(64), 0, s, h->dc, B, Nsim, x0, U, X, pt...);
    });
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

extern "C" int mpc_rollout_held(mpc_handle *h, int B, const double *x, const double *U, const int32_t *held, double *X, void *stream)
{
    int rc = check_common(h, B, "mpc_rollout_held"); if (rc) return rc;
    if (B == 0) return MPC_OK;
    if (!x || !U || !held || !X) return fail(MPC_E_ARG, "mpc_rollout_held: null buffer");
    rc = check_tables(h, B, "mpc_rollout_held", READS_PARAMS); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    with_model_table(h, h->params().idx, [&](auto MODEL, auto PA, auto... pt) {
        hipLaunchKernelGGL((simulate_held_kernel<MODEL(), PA(), decltype(pt)...>), grid_for(B, 64), dim3(64), 0, s, h->dc, B, x, U, held, X, pt...);
    });
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

extern "C" int mpc_stage_errors(mpc_handle *h, int B, const double *pose, const double *cl,
                                const int32_t *cl_index, double *err, int32_t *idx, void *stream)
{
    int rc = check_common(h, B, "mpc_stage_errors"); if (rc) return rc;
    if (B == 0) return MPC_OK;
    if (!pose || !cl || !err) return fail(MPC_E_ARG, "mpc_stage_errors: null buffer");
    hipLaunchKernelGGL(errors_kernel, grid_for(B, 64), dim3(64), 0, (hipStream_t)stream, h->dc, B, pose, cl,
                       cl_index, near_for(h, cl), err, idx);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

extern "C" int mpc_lane_payoff(mpc_handle *h, int B, int K, const double *params15, const double *ego,
                               const double *cars, const int32_t *ncars, double *out, void *stream)
{
    int rc = check_common(h, B, "mpc_lane_payoff"); if (rc) return rc;
    if (B == 0) return MPC_OK;
    if (K < 0 || K > 62 || !params15 || !ego || (K > 0 && !cars) || !ncars || !out)
        return fail(MPC_E_ARG, "mpc_lane_payoff: bad argument");
    LaneParams p;
    std::memcpy(&p, params15, sizeof p); // host array of 15 doubles
    hipLaunchKernelGGL(lane_payoff_kernel, grid_for(B, 64), dim3(64), 0, (hipStream_t)stream, p, B, K, ego, cars,
                       ncars, out);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

extern "C" int mpc_math_probe(mpc_handle *h, int n, int op, const double *a, const double *b, double *out,
                              void *stream)
{
    int rc = check_common(h, n, "mpc_math_probe"); if (rc) return rc;
    if (n == 0) return MPC_OK;
    if (!a || !out || (op == 3 && !b)) return fail(MPC_E_ARG, "mpc_math_probe: null buffer");
    hipLaunchKernelGGL(math_probe_kernel, grid_for(n, 256), dim3(256), 0, (hipStream_t)stream, n, op, a, b, out);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

extern "C" int mpc_stage_cost(mpc_handle *h, int B, const double *x, const double *u, const double *cl,
                              const int32_t *cl_index, double *out, void *stream)
{
    int rc = check_common(h, B, "mpc_stage_cost"); if (rc) return rc;
    if (B == 0) return MPC_OK;
    if (!x || !u || !cl || !out) return fail(MPC_E_ARG, "mpc_stage_cost: null buffer");
    rc = check_tables(h, B, "mpc_stage_cost", READS_PARAMS); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    with_model_table(h, h->params().idx, [&](auto MODEL, auto PA, auto... pt) {
        hipLaunchKernelGGL((stage_cost_kernel<MODEL(), PA(), decltype(pt)...>), grid_for(B, 64), dim3(64), 0, s,
                           h->dc, B, x, u, cl, cl_index, out, pt...);
    });
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

static int eval_cost_grad(mpc_handle *h, int B, const double *x0, const double *cl, const int32_t *cl_index,
                          const double *U, const double *y, const double *Sigma, double *psi, double *grad,
                          double *yhat, void *stream, bool wave_path, const double *U2 = nullptr, double *grad2 = nullptr)
{
    int rc = check_common(h, B, "mpc_eval_cost_grad"); if (rc) return rc;
    if (B == 0) return MPC_OK;
    if (!x0 || !cl || !U || !psi) return fail(MPC_E_ARG, "mpc_eval_cost_grad: null buffer");
    const DevCfg &c = h->dc;
    if (c.m && (!y || !Sigma)) return fail(MPC_E_ARG, "mpc_eval_cost_grad: y and Sigma are required when m > 0");
    rc = check_tables(h, B, "mpc_eval_cost_grad", READS_PARAMS | READS_CONSTR | READS_DISCS | READS_RATES | READS_FIELDS | READS_ROADS, true); if (rc) return rc;
    rc = reserve(h, B); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    // direct mode: the kernel reads and writes the caller's agent-major buffers in place
    WorkspaceHost w = h->ws;
    w.cl = cl; w.cl_index = cl_index; w.x0 = x0; w.near = near_for(h, cl);
    w.xe = const_cast<double *>(U); w.ge = grad ? grad : h->ws.ws_ge;
    w.y = const_cast<double *>(y); w.Sig = c.m ? const_cast<double *>(Sigma) : h->ws.ws_Sig;
    w.yhe = (yhat && c.m) ? yhat : h->ws.ws_yhe;
    w.psi_direct = psi;
    if (U2) { w.xe2 = const_cast<double *>(U2); w.ge2 = grad2; }
    h->bind_tables(w, h->bound_rows());
    if (wave_path) launch_solo_eval(h, w, s, (grad ? 1 : 0) | (U2 ? 2 : 0));
    else launch_eval(h, w, s, nullptr, nullptr, grad ? B : 0, grad ? 0 : B);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}
extern "C" int mpc_eval_cost_grad(mpc_handle *h, int B, const double *x0, const double *cl, const int32_t *cl_index, const double *U,
                                  const double *y, const double *Sigma, double *psi, double *grad, double *yhat, void *stream)
{
    return eval_cost_grad(h, B, x0, cl, cl_index, U, y, Sigma, psi, grad, yhat, stream, false);
}
extern "C" int mpc_eval_cost_grad_wave(mpc_handle *h, int B, const double *x0, const double *cl, const int32_t *cl_index, const double *U,
                                       const double *y, const double *Sigma, double *psi, double *grad, double *yhat, void *stream)
{
    return eval_cost_grad(h, B, x0, cl, cl_index, U, y, Sigma, psi, grad, yhat, stream, true);
}

// Two points, one trip: the evaluation at U (cost, and gradient when grad is given) and the gradient at U2 side by side
// in one wave, as a trip of the kinematic persistent kernel that carries a speculative gradient runs them (solo_halves:
// nfe = 4, horizons of at most half a wave).
extern "C" int mpc_eval_cost_grad_wave2(mpc_handle *h, int B, const double *x0, const double *cl, const int32_t *cl_index, const double *U,
                                        const double *U2, const double *y, const double *Sigma, double *psi, double *grad, double *grad2,
                                        double *yhat, void *stream)
{
    int rc = check_common(h, B, "mpc_eval_cost_grad_wave2"); if (rc) return rc;
    if (B == 0) return MPC_OK;
    if (!U2 || !grad2) return fail(MPC_E_ARG, "mpc_eval_cost_grad_wave2: null buffer");
    if (!solo_halves(h->dc.model, h->dc.nfe, h->dc.N))
        return fail(MPC_E_ARG, "mpc_eval_cost_grad_wave2: the kinematic model with nfe = 4 and N <= 32 (the half-wave form of the wide rollout)");
    return eval_cost_grad(h, B, x0, cl, cl_index, U, y, Sigma, psi, grad, yhat, stream, true, U2, grad2);
}

extern "C" int mpc_prox_step(mpc_handle *h, int B, const double *x, const double *grad, const double *gamma,
                             double *xhat, double *p, double *out, void *stream)
{
    int rc = check_common(h, B, "mpc_prox_step"); if (rc) return rc;
    if (B == 0) return MPC_OK;
    if (!x || !grad || !gamma || !out) return fail(MPC_E_ARG, "mpc_prox_step: null buffer");
    rc = check_tables(h, B, "mpc_prox_step", READS_BOX); if (rc) return rc;
    const auto launch = [&](auto... t) {
        hipLaunchKernelGGL((prox_kernel<decltype(t)...>), grid_for(B, 64), dim3(64), 0, (hipStream_t)stream, h->dc, B, x, grad, gamma, xhat, p,
                           out, t...);
    };
    if (const BoundTable &box = h->tab[TAB_BOX]; box.table) launch(BoxTab{box.table, box.idx});
    else launch();
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

extern "C" int mpc_lbfgs_apply(mpc_handle *h, int B, const double *S, const double *Y, const int32_t *idx,
                               const int32_t *full, const double *mask, double *q, int32_t *ok, void *stream)
{
    int rc = check_common(h, B, "mpc_lbfgs_apply"); if (rc) return rc;
    if (B == 0) return MPC_OK;
    if (!S || !Y || !idx || !full || !mask || !q || !ok) return fail(MPC_E_ARG, "mpc_lbfgs_apply: null buffer");
    rc = reserve(h, B); if (rc) return rc;
    const DevCfg &c = h->dc;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *rows = h->ws.totals + 3;
    with_flag(c.n > 64, [&](auto TWO) {   // elements per lane, as with_hist_variant; the history always from global memory
        hipLaunchKernelGGL((lbfgs_apply_kernel<TWO() ? 2 : 1, 0>), dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, c, B, S, Y, idx, full, mask, q, ok, rows);
    });
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

extern "C" int mpc_step_lds_plan(int n, int M, int m, int chain, int lds_pairs, int *pairs, int *lds_bytes, int *waves_per_simd)
{
    if (n < 1 || M < 1 || m < 0 || !pairs || !lds_bytes || !waves_per_simd) return fail(MPC_E_ARG, "mpc_step_lds_plan: bad argument");
    int ne = 0;   // (the plan is that of the variant with the LDS copy)
    with_hist_variant<false>(n, M, false, [&](auto NE, auto) { ne = NE(); });
    *pairs = step_lds_pairs(ne, n, M, m, lds_pairs);
    *lds_bytes = (int)step_dyn_lds(ne, n, *pairs, chain != 0);
    *waves_per_simd = step_waves_per_simd(ne, -1, m != 0);
    return MPC_OK;
}

// the solve proper on B agents whose rows of the bound tables are idx.of[kind][b] (a kind with no table bound: not
// read): the caller's batch and the handle's bound indices (mpc_solve_batch), or the gathered rows of a masked solve and
// their gathered indices
static int solve_core(mpc_handle *h, int B, const double *x0, const double *cl, const int32_t *cl_index, const AgentIdx &idx,
                      double *U, double *lambda, double *stats, hipStream_t s)
{
    int rc = reserve(h, B); if (rc) return rc;
    WorkspaceHost &w = h->ws;
    w.cl = cl; w.cl_index = cl_index; w.x0 = x0; w.xo = U; w.y = lambda; w.psi_direct = nullptr;
    w.near = near_for(h, cl);
    h->bind_tables(w, idx);
    w.xe = w.ws_xe; w.ge = w.ws_ge; w.yhe = w.ws_yhe; w.Sig = w.ws_Sig;
    rc = run_solver(h, s); if (rc) return rc;
    if (stats) hipLaunchKernelGGL(stats_kernel, grid_for(B, 256), dim3(256), 0, s, w, stats);
    HIPCHK(hipGetLastError());
    return bounded_sync(h, s, "mpc_solve_batch");
}
static int solve_batch_impl(mpc_handle *h, int B, const double *x0, const double *cl, const int32_t *cl_index,
                            double *U, double *lambda, double *stats, void *stream, bool from_worker)
{
    int rc = check_common(h, B, "mpc_solve_batch", from_worker); if (rc) return rc;
    if (B == 0) return MPC_OK;
    if (!x0 || !cl || !U) return fail(MPC_E_ARG, "mpc_solve_batch: null buffer");
    if (h->dc.m && !lambda) return fail(MPC_E_ARG, "mpc_solve_batch: lambda is required when m > 0");
    rc = check_tables(h, B, "mpc_solve_batch", READS_ALL, true); if (rc) return rc;
    return solve_core(h, B, x0, cl, cl_index, h->bound_rows(), U, lambda, stats, (hipStream_t)stream);
}
extern "C" int mpc_solve_batch(mpc_handle *h, int B, const double *x0, const double *cl, const int32_t *cl_index, double *U,
                               double *lambda, double *stats, void *stream)
{
    return solve_batch_impl(h, B, x0, cl, cl_index, U, lambda, stats, stream, false);
}

// The round loop of a solve is host code (launches, counter polls): the asynchronous form runs it on a
// worker thread owned by the handle, so the caller gets its thread back at once and may run a second
// handle's solve, or its own work, beside it.  One solve in flight per handle.
static void async_worker(mpc_handle *h)
{
    for (;;) {
        mpc_handle::AsyncJob j;
        {
            std::unique_lock<std::mutex> lk(h->mu);
            h->cv.wait(lk, [&] { return h->job_posted || h->worker_quit; });
            if (!h->job_posted) return;   // quit
            j = h->job; h->job_posted = false; h->job_running = true;
        }
        const int rc = solve_batch_impl(h, j.B, j.x0, j.cl, j.cl_index, j.U, j.lambda, j.stats, j.stream, true);
        {
            std::lock_guard<std::mutex> lk(h->mu);
            h->job_rc = rc; h->job_err = rc ? g_err : std::string();
            h->job_running = false; h->job_done = true;
        }
        h->cv.notify_all();
    }
}

extern "C" int mpc_solve_batch_async(mpc_handle *h, int B, const double *x0, const double *cl,
                                     const int32_t *cl_index, double *U, double *lambda, double *stats,
                                     void *stream)
{
    if (!h) return fail(MPC_E_ARG, "mpc_solve_batch_async: null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->job_posted || h->job_running || h->job_done)
        return fail(MPC_E_ARG, "mpc_solve_batch_async: a solve of this handle is in flight (mpc_solve_wait first)");
    if (!h->worker.joinable()) h->worker = std::thread(async_worker, h);
    h->job = {B, x0, cl, cl_index, U, lambda, stats, stream};
    h->job_posted = true;
    h->cv.notify_all();
    return MPC_OK;
}

extern "C" int mpc_solve_wait(mpc_handle *h)
{
    if (!h) return fail(MPC_E_ARG, "mpc_solve_wait: null handle");
    std::unique_lock<std::mutex> lk(h->mu);
    if (!h->job_posted && !h->job_running && !h->job_done) return fail(MPC_E_ARG, "mpc_solve_wait: no solve in flight");
    h->cv.wait(lk, [&] { return h->job_done; });
    h->job_done = false;
    if (h->job_rc != MPC_OK) g_err = h->job_err;
    return h->job_rc;
}

extern "C" int mpc_closed_loop(mpc_handle *h, int B, int T, int shift, double *x, const double *cl,
                               const int32_t *cl_index, double *U, double *lambda, double *traj_x,
                               double *traj_u, int32_t *fail_count, double *stats, void *stream)
{
    int rc = check_common(h, B, "mpc_closed_loop"); if (rc) return rc;
    if (B == 0 || T == 0) return MPC_OK;
    if (T < 0 || !x || !cl || !U) return fail(MPC_E_ARG, "mpc_closed_loop: bad argument");
    const DevCfg &c = h->dc;
    if (c.m && !lambda) return fail(MPC_E_ARG, "mpc_closed_loop: lambda is required when m > 0");
    rc = check_tables(h, B, "mpc_closed_loop", READS_ALL, true); if (rc) return rc;
    rc = check_rate_rows(h, B, "mpc_closed_loop"); if (rc) return rc;
    const auto nothing = [](int) -> int { return MPC_OK; };
    rc = plant_loop(h, B, T, shift, x, cl, cl_index, U, lambda, traj_x, traj_u, fail_count, stats, stream, nothing, nothing);
    if (rc) return rc;
    // (a plain wait here, bounded_sync in every other loop: they differ in what a device that stops answering does to the
    // call; making them one is left to a change of its own)
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return MPC_OK;
}

// The masked solve, by compaction: list the active agents (index-ascending, two passes, no atomics), gather their rows
// into the handle's staging buffers, run the solve that mpc_solve_batch runs on those n_active agents, scatter U,
// lambda and stats back.  The solver kernels see a plain batch; the rows of the other agents are never written.  The
// count reaches the host behind the gather through pinned memory and the bounded wait every solve uses.
static int solve_active_impl(mpc_handle *h, int B, const int32_t *active, const double *x0, const double *cl,
                             const int32_t *cl_index, double *U, double *lambda, double *stats, int32_t *n_active,
                             hipStream_t s, bool final_sync)
{
    int rc = reserve_event(h, B); if (rc) return rc;
    const DevCfg &c = h->dc;
    EventBufs &e = h->ev;
    const dim3 gblk = grid_for(B, EV_BLK), grows = grid_for(B, EV_BLK / 64);
    hipLaunchKernelGGL(active_count_kernel, gblk, dim3(EV_BLK), 0, s, B, active, e.blk);
    hipLaunchKernelGGL(active_list_kernel, gblk, dim3(EV_BLK), 0, s, B, active, e.blk, e.list, e.count);
    ActiveRows r;
    r.list = e.list; r.count = e.count; r.nx = c.nx; r.n = c.n; r.m = c.m;
    r.x0 = const_cast<double *>(x0); r.U = U; r.lam = lambda; r.stats = stats;
    r.cl_index = cl_index; r.pidx = h->params().idx;
    r.xs = e.xs; r.Us = e.Us; r.lams = e.lams; r.stats_s = e.stats_s; r.cis = e.cis; r.pis = e.rows[TAB_PARAMS];
    hipLaunchKernelGGL(active_gather_kernel, grows, dim3(EV_BLK), 0, s, r);
    AgentIdx gathered;
    for (int k = 0; k < TAB_KINDS; k++) gathered.of[k] = e.rows[k];
    for (int k = TAB_BOX; k < TAB_KINDS; k++)   // (the parameter rows ride in the gather above)
        if (h->tab[k].table)
            hipLaunchKernelGGL(active_index_kernel, gblk, dim3(EV_BLK), 0, s, e.list, e.count, h->tab[k].idx, e.rows[k]);
    int *cnt = &h->pinned().n_active;
    HIPCHK(hipMemcpyAsync(cnt, e.count, sizeof(int), hipMemcpyDeviceToHost, s));
    rc = bounded_sync(h, s, "mpc_solve_active"); if (rc) return rc;
    const int nA = *cnt;
    if (nA < 0 || nA > B) return fail(MPC_E_HIP, "mpc_solve_active: the compaction counted " + std::to_string(nA) + " of " + std::to_string(B) + " agents");
    if (n_active) *n_active = nA;
    if (nA == 0) return MPC_OK;
    rc = solve_core(h, nA, e.xs, cl, cl_index ? e.cis : nullptr, gathered, e.Us, c.m ? e.lams : nullptr,
                    stats ? e.stats_s : nullptr, s);
    if (rc) return rc;
    hipLaunchKernelGGL(active_scatter_kernel, grid_for(nA, EV_BLK / 64), dim3(EV_BLK), 0, s, r);
    HIPCHK(hipGetLastError());
    return final_sync ? bounded_sync(h, s, "mpc_solve_active") : MPC_OK;
}

extern "C" int mpc_solve_active(mpc_handle *h, int B, const int32_t *active, const double *x0, const double *cl,
                                const int32_t *cl_index, double *U, double *lambda, double *stats, int32_t *n_active,
                                void *stream)
{
    if (n_active) *n_active = 0;
    int rc = check_common(h, B, "mpc_solve_active"); if (rc) return rc;
    if (B == 0) return MPC_OK;
    if (!active || !x0 || !cl || !U) return fail(MPC_E_ARG, "mpc_solve_active: null buffer");
    if (h->dc.m && !lambda) return fail(MPC_E_ARG, "mpc_solve_active: lambda is required when m > 0");
    rc = check_tables(h, B, "mpc_solve_active", READS_ALL, true); if (rc) return rc;   // the caller's B; the compact batch is the library's
    return solve_active_impl(h, B, active, x0, cl, cl_index, U, lambda, stats, n_active, (hipStream_t)stream, true);
}

// what mpc_trigger_eval and mpc_closed_loop_event ask of the trigger's arguments, checked before anything else (and so
// without a device); max_hold <= N needs the handle and is checked behind its null test
static int check_trigger_args(const char *who, const double *w, double thr, int max_hold, const void *held)
{
    if (!w || !held) return fail(MPC_E_ARG, std::string(who) + ": null w or held");
    if (!(thr >= 0.0)) return fail(MPC_E_ARG, std::string(who) + ": thr must be >= 0 (+inf: the hold limit alone)");
    if (max_hold < 1) return fail(MPC_E_ARG, std::string(who) + ": max_hold must be in [1, N]");
    return MPC_OK;
}
static int check_max_hold(const mpc_handle *h, const char *who, int max_hold)
{
    if (max_hold > h->cfg.N) return fail(MPC_E_ARG, std::string(who) + ": max_hold must be in [1, N]");
    return MPC_OK;
}
static TrigW trigger_weights(const mpc_handle *h, const double *w)
{
    TrigW tw{};
    for (int i = 0; i < h->dc.nx; i++) tw.w[i] = w[i];
    return tw;
}
static void launch_trigger(mpc_handle *h, hipStream_t s, int B, const double *x, const double *xhat, const int32_t *held,
                           const TrigW &tw, double thr, int max_hold, int force, double *dev2, int32_t *fire, double *U)
{
    with_model(h->dc.model, [&](auto MODEL) {
        hipLaunchKernelGGL((trigger_kernel<ModelDim<MODEL()>::NX>), grid_for(B, 64), dim3(64), 0, s, B, h->dc.N, x, xhat, held, tw,
                           thr * thr, max_hold, force, dev2, fire, U);
    });
}

extern "C" int mpc_trigger_eval(mpc_handle *h, int B, const double *x, const double *xhat, const int32_t *held,
                                const double *w, double thr, int max_hold, double *dev2, int32_t *fire, void *stream)
{
    int rc = check_trigger_args("mpc_trigger_eval", w, thr, max_hold, held); if (rc) return rc;
    if (!h) return fail(MPC_E_ARG, "mpc_trigger_eval: null handle");
    rc = check_max_hold(h, "mpc_trigger_eval", max_hold); if (rc) return rc;
    rc = check_common(h, B, "mpc_trigger_eval"); if (rc) return rc;
    if (B == 0) return MPC_OK;
    if (!x || !xhat || !fire) return fail(MPC_E_ARG, "mpc_trigger_eval: null buffer");
    launch_trigger(h, (hipStream_t)stream, B, x, xhat, held, trigger_weights(h, w), thr, max_hold, 0, dev2, fire, nullptr);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

// ---------------------------------------------------------------------------------- lap driving (mpc_track.hpp)
// windows of a track of L points with stride w: closed ceil(L / w), open (L - S) / w + 1; -1 when L < S
static long long track_window_count(long long L, long long S, long long w, int closed)
{
    if (L < S || w < 1) return -1;
    return closed ? (L + w - 1) / w : (L - S) / w + 1;
}
extern "C" int mpc_track_init(mpc_track *t, const mpc_config *cfg, int K, int L, int stride, int lead, int closed)
{
    if (!t || !cfg) return fail(MPC_E_ARG, "mpc_track_init: null argument");
    const int S = cfg->S;
    if (S < 3) return fail(MPC_E_ARG, "mpc_track_init: the configuration needs S >= 3 centerline points");
    if (K < 1) return fail(MPC_E_ARG, "mpc_track_init: K must be >= 1");
    if (L < S) return fail(MPC_E_ARG, "mpc_track_init: a track needs L >= S = " + std::to_string(S) + " points");
    if (stride < 1) return fail(MPC_E_ARG, "mpc_track_init: stride must be >= 1");
    if (lead < 0 || lead > S - 2) return fail(MPC_E_ARG, "mpc_track_init: lead must be in [0, S - 2]");
    const long long R = track_window_count(L, S, stride, closed);
    if (R < 1 || (long long)K * R > 2147483647ll) return fail(MPC_E_ARG, "mpc_track_init: K * R does not fit an int32");
    t->K = K; t->L = L; t->stride = stride; t->lead = lead; t->closed = closed ? 1 : 0; t->R = (int32_t)R;
    return MPC_OK;
}
// a track as mpc_track_init fills it for this handle's S (anything else is refused before a kernel sees it)
static int check_track(const mpc_handle *h, const mpc_track *t, const char *who)
{
    if (!t) return fail(MPC_E_ARG, std::string(who) + ": null track");
    const int S = h->cfg.S;
    const long long R = track_window_count(t->L, S, t->stride, t->closed);
    if (t->K < 1 || R < 1 || t->lead < 0 || t->lead > S - 2 || (t->closed != 0 && t->closed != 1) || R != t->R ||
        (long long)t->K * R > 2147483647ll)
        return fail(MPC_E_ARG, std::string(who) + ": the track's geometry is not what mpc_track_init gives for this handle");
    return MPC_OK;
}
static TrackGeom track_geom(const mpc_track *t) { return TrackGeom{t->K, t->L, t->stride, t->lead, t->closed, t->R}; }

extern "C" int mpc_track_windows(mpc_handle *h, const mpc_track *t, const double *track, double *win, void *stream)
{
    int rc = check_common(h, 0, "mpc_track_windows"); if (rc) return rc;
    rc = check_track(h, t, "mpc_track_windows"); if (rc) return rc;
    if (!track || !win) return fail(MPC_E_ARG, "mpc_track_windows: null buffer");
    const size_t words = (size_t)t->K * (size_t)t->R * 2 * (size_t)h->cfg.S;
    const unsigned blocks = (unsigned)std::min<size_t>((words + 255) / 256, (size_t)1 << 20);
    hipLaunchKernelGGL(track_windows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, track_geom(t), h->cfg.S, track, win);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

// what the two per-agent calls share: the handle, the track and, with tables bound, the batch they are bound for
static int check_track_call(mpc_handle *h, const mpc_track *t, int B, const char *who)
{
    int rc = check_common(h, B, who); if (rc) return rc;
    rc = check_track(h, t, who); if (rc) return rc;
    return check_tables(h, B, who, READS_ALL);
}

extern "C" int mpc_track_locate(mpc_handle *h, const mpc_track *t, int B, const double *x, const double *track,
                                const int32_t *track_index, int32_t *cl_index, void *stream)
{
    int rc = check_track_call(h, t, B, "mpc_track_locate"); if (rc) return rc;
    if (B == 0) return MPC_OK;
    if (!x || !track || !cl_index) return fail(MPC_E_ARG, "mpc_track_locate: null buffer");
    DevCfg cL = h->dc;
    cL.S = t->L;                           // nearest_index over the whole track row: candidates 0 .. L-2
    hipLaunchKernelGGL(track_locate_kernel, grid_for(B, 64), dim3(64), 0, (hipStream_t)stream, cL, track_geom(t), B, h->dc.nx, x,
                       track, track_index, cl_index);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

extern "C" int mpc_track_select(mpc_handle *h, const mpc_track *t, int B, const double *x, const double *win,
                                const int32_t *active, int32_t *cl_index, int32_t *pos, void *stream)
{
    int rc = check_track_call(h, t, B, "mpc_track_select"); if (rc) return rc;
    if (B == 0) return MPC_OK;
    if (!x || !win || !cl_index) return fail(MPC_E_ARG, "mpc_track_select: null buffer");
    hipLaunchKernelGGL(track_select_kernel, grid_for(B, 64), dim3(64), 0, (hipStream_t)stream, h->dc, track_geom(t), B, h->dc.nx, x,
                       win, active, near_for(h, win), cl_index, pos, (int *)nullptr, 0, 0);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

// Event-triggered closed loop: per step the trigger (which also shifts a firing agent's plan by the stages it has
// applied), the masked solve of the agents that fired, and one kernel that applies stage `held` of every agent's plan
// to plant and nominal state.  Control returns to the host once per step for the count of firing agents (and, inside
// the solve, once per round window, as in every solve); data never leaves the device.
// (trk != null: mpc_closed_loop_track -- between the trigger and the masked solve the firing agents re-select their row
// of the window table `cl` on the plant state, and traj_row records the row in force; trk == null launches nothing more)
// (Hook::on: mpc_closed_loop_obstacles_event -- the trigger leaves the plans alone and hook.fired(t, fire) (the obstacle rule on
// top of fire, then the shift) runs behind it, hook.selected (the selection and the firing agents' rows) behind the track's
// re-selection and before the solve, hook.stepped (the realised clearance) behind the step; each returns an rc, as
// plant_loop's before and after do.  NoEventHook launches nothing more.)
struct NoEventHook { static constexpr bool on = false; };
template <class Hook = NoEventHook>
static int closed_loop_event_impl(const char *who_, mpc_handle *h, int B, int T, int shift, const double *w, double thr, int max_hold,
                                  double *x, const double *cl, const int32_t *cl_index, double *U, double *lambda,
                                  int32_t *held, const double *disturbance, double *traj_x, double *traj_u,
                                  uint8_t *solved, int32_t *solve_count, int32_t *fail_count, double *stats, void *stream,
                                  const mpc_track *trk, int32_t *cl_index_rw, int32_t *traj_row, const Hook &hook = Hook())
{
    const std::string who(who_);
    int rc = check_trigger_args(who_, w, thr, max_hold, held); if (rc) return rc;
    if (T < 0) return fail(MPC_E_ARG, who + ": negative T");
    if (!h) return fail(MPC_E_ARG, who + ": null handle");
    rc = check_max_hold(h, who_, max_hold); if (rc) return rc;
    rc = check_common(h, B, who_); if (rc) return rc;
    if (trk) { rc = check_track(h, trk, who_); if (rc) return rc; }
    if (B == 0 || T == 0) return MPC_OK;
    if (!x || !cl || !U || (trk && !cl_index_rw)) return fail(MPC_E_ARG, who + ": null buffer");
    const DevCfg &c = h->dc;
    if (c.m && !lambda) return fail(MPC_E_ARG, who + ": lambda is required when m > 0");
    rc = check_tables(h, B, who_, READS_ALL, true); if (rc) return rc;
    rc = check_rate_rows(h, B, who); if (rc) return rc;
    rc = reserve_event(h, B); if (rc) return rc;
    bool fresh = false;
    rc = reserve_xhat(h, B, &fresh); if (rc) return rc;
    EventBufs &e = h->ev;
    hipStream_t s = (hipStream_t)stream;
    double *st = stats ? stats : e.stats_own;
    const TrigW tw = trigger_weights(h, w);
    for (int t = 0; t < T; t++) {
        // (nominal states just allocated: every agent re-plans at the first step, whatever `held` says)
        launch_trigger(h, s, B, x, e.xhat, held, tw, thr, max_hold, fresh && t == 0, nullptr, e.fire, shift && !Hook::on ? U : nullptr);
        if constexpr (Hook::on) { rc = hook.fired(t, e.fire); if (rc) return rc; }
        if (trk)
            hipLaunchKernelGGL(track_select_kernel, grid_for(B, 64), dim3(64), 0, s, c, track_geom(trk), B, c.nx, x, cl, e.fire,
                               near_for(h, cl), cl_index_rw, (int *)nullptr, traj_row, t, T);
        if constexpr (Hook::on) { rc = hook.selected(t, e.fire); if (rc) return rc; }
        rc = solve_active_impl(h, B, e.fire, x, cl, cl_index, U, lambda, st, nullptr, s, false); if (rc) return rc;
        launch_rate_prev(h, s, B, U, held, e.fire);
        // bound table: the plant advances with row pidx_plant[b] (null: the controller's), the nominal state with pidx[b]
        with_model_table(h, h->plant_rows(), [&](auto MODEL, auto PA, auto... pt) {
            if constexpr (PA())
                hipLaunchKernelGGL((event_step_kernel<MODEL(), true, decltype(pt)..., const int32_t *>), grid_for(B, 64), dim3(64), 0, s,
                                   c, B, t, T, x, e.xhat, U, held, e.fire, disturbance, traj_x, traj_u, solved, solve_count,
                                   st, fail_count, pt..., h->params().idx);
            else
                hipLaunchKernelGGL((event_step_kernel<MODEL(), false>), grid_for(B, 64), dim3(64), 0, s,
                                   c, B, t, T, x, e.xhat, U, held, e.fire, disturbance, traj_x, traj_u, solved, solve_count,
                                   st, fail_count);
        });
        if constexpr (Hook::on) { rc = hook.stepped(t, e.fire); if (rc) return rc; }
    }
    HIPCHK(hipGetLastError());
    return bounded_sync(h, s, who_);
}
extern "C" int mpc_closed_loop_event(mpc_handle *h, int B, int T, int shift, const double *w, double thr, int max_hold,
                                     double *x, const double *cl, const int32_t *cl_index, double *U, double *lambda,
                                     int32_t *held, const double *disturbance, double *traj_x, double *traj_u,
                                     uint8_t *solved, int32_t *solve_count, int32_t *fail_count, double *stats, void *stream)
{
    return closed_loop_event_impl("mpc_closed_loop_event", h, B, T, shift, w, thr, max_hold, x, cl, cl_index, U, lambda, held,
                                  disturbance, traj_x, traj_u, solved, solve_count, fail_count, stats, stream, nullptr, nullptr, nullptr);
}

// Lap driving: the event-triggered loop on a table of track windows, every firing agent re-selecting its row
extern "C" int mpc_closed_loop_track(mpc_handle *h, int B, int T, int shift, const double *w, double thr, int max_hold,
                                     double *x, const double *win, int32_t *cl_index, double *U, double *lambda,
                                     int32_t *held, const double *disturbance, double *traj_x, double *traj_u,
                                     uint8_t *solved, int32_t *solve_count, int32_t *fail_count, double *stats, void *stream,
                                     const mpc_track *trk, int32_t *traj_row)
{
    if (!trk) return fail(MPC_E_ARG, "mpc_closed_loop_track: null track");
    return closed_loop_event_impl("mpc_closed_loop_track", h, B, T, shift, w, thr, max_hold, x, win, cl_index, U, lambda, held,
                                  disturbance, traj_x, traj_u, solved, solve_count, fail_count, stats, stream, trk, cl_index, traj_row);
}

// ---------------------------------------------------------------------------------- traffic (mpc_traffic.hpp)
static_assert(MPC_SCENE_MAX == mpc::SCENE_MAX, "scene size: include/mpc_hip.h and mpc_traffic.hpp");
// what mpc_opponents_from_plans and mpc_closed_loop_traffic ask of the scene arguments (checked without a device)
static int check_scene_args(const std::string &who, int B, int G, double reach, const void *radius)
{
    if (G < 1 || G > MPC_SCENE_MAX) return fail(MPC_E_ARG, who + ": the scene size G must be in [1, " + std::to_string(MPC_SCENE_MAX) + "]");
    if (B < 0) return fail(MPC_E_ARG, who + ": negative batch");
    if (B % G) return fail(MPC_E_ARG, who + ": the batch of " + std::to_string(B) + " agents is not a whole number of scenes of G = " +
                                       std::to_string(G) + " (B % G != 0: pad the scenes)");
    if (!(reach >= 0.0)) return fail(MPC_E_ARG, who + ": reach must be >= 0 (+inf: every agent of the scene)");
    if (!radius) return fail(MPC_E_ARG, who + ": null radius");
    return MPC_OK;
}
// the selection on plans X [B][Nst][nx] (see opponents_kernel for the three outputs)
// (held != null: the held form -- agent b compares the stages a plan of Nst of which held[b] are applied still holds)
static void launch_opponents(mpc_handle *h, hipStream_t s, int B, int G, int Nst, const double *X, const double *radius, double reach,
                             int32_t *opp, int32_t *opp_rec, size_t rec_stride, double *clear, size_t clear_stride, int clear_slots,
                             const int32_t *held = nullptr)
{
    int Gp = 1;
    while (Gp < G) Gp <<= 1;
    const int spw = 64 / Gp, scenes = B / G;
    const dim3 grid((unsigned)((scenes + spw - 1) / spw));
    if (held)
        hipLaunchKernelGGL((opponents_kernel<true, const int32_t *>), grid, dim3(TR_BLK), 0, s, B, G, Gp, spw, Nst, h->dc.nx, X, radius,
                           reach * reach, opp, opp_rec, rec_stride, clear, clear_stride, clear_slots, held);
    else
        hipLaunchKernelGGL(opponents_kernel<>, grid, dim3(TR_BLK), 0, s, B, G, Gp, spw, Nst, h->dc.nx, X, radius, reach * reach, opp,
                           opp_rec, rec_stride, clear, clear_stride, clear_slots);
}

extern "C" int mpc_opponents_from_plans(mpc_handle *h, int B, int G, int Nst, const double *X, const double *radius, double reach,
                                        int32_t *opp, double *clear, void *stream)
{
    const char *who = "mpc_opponents_from_plans";
    int rc = check_scene_args(who, B, G, reach, radius); if (rc) return rc;
    if (Nst < 1) return fail(MPC_E_ARG, std::string(who) + ": Nst must be >= 1 stages");
    if (!X || !opp) return fail(MPC_E_ARG, std::string(who) + ": null X or opp");
    rc = check_common(h, B, who); if (rc) return rc;
    rc = check_tables(h, B, who, READS_ALL); if (rc) return rc;
    if (B == 0) return MPC_OK;
    launch_opponents(h, (hipStream_t)stream, B, G, Nst, X, radius, reach, opp, nullptr, 0, clear, MPC_NDISC, MPC_NDISC);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

// Traffic closed loop: per step everybody's plans (mpc_rollout), the nearest opponents of every agent on them, their
// discs into the bound table (mpc_discs_from_plans) -- or their risk fields (mpc_fields_from_plans:
// mpc_closed_loop_traffic_field) -- the solve, the plant step of mpc_closed_loop, and the clearance realised on the new
// states.  Every step is what the public call of that name launches; control returns to the host inside the solve alone.
// One body for the two loops: `kind` is the table the loop rewrites (TAB_DISCS or TAB_FIELDS), `gather` step 3.
template <class Gather>
static int closed_loop_traffic_impl(const std::string &who, TableKind kind, mpc_handle *h, int B, int T, int shift, int G, const double *radius,
                                    double reach, double *x, const double *cl, const int32_t *cl_index, double *U, double *lambda,
                                    double *table, double *traj_x, double *traj_u, int32_t *traj_opp, double *traj_clear,
                                    int32_t *fail_count, double *stats, void *stream, Gather gather)
{
    int rc = check_tables(h, B, who.c_str(), READS_ALL, true); if (rc) return rc;
    rc = check_rewritten_table(h, kind, table, B, who); if (rc) return rc;
    rc = check_rate_rows(h, B, who); if (rc) return rc;
    if (B == 0 || T == 0) return MPC_OK;
    if (!x || !cl || !U || (h->dc.m && !lambda)) return fail(MPC_E_ARG, who + ": null buffer");
    rc = reserve_traffic(h, B); if (rc) return rc;
    const int N = h->dc.N;
    TrafficBufs &tr = h->tr;
    hipStream_t s = (hipStream_t)stream;
    const auto before = [&](int t) -> int {
        const int rr = mpc_rollout(h, B, N, x, U, tr.X, stream); if (rr) return rr;
        launch_opponents(h, s, B, G, N, tr.X, radius, reach, tr.opp, traj_opp ? traj_opp + (size_t)t * MPC_NDISC : nullptr,
                         (size_t)T * MPC_NDISC, nullptr, 0, 0);
        return gather(tr.X, tr.opp);
    };
    const auto after = [&](int t) -> int {
        if (traj_clear) launch_opponents(h, s, B, G, 1, x, radius, INFINITY, nullptr, nullptr, 0, traj_clear + t, (size_t)T, 1);
        return MPC_OK;
    };
    rc = plant_loop(h, B, T, shift, x, cl, cl_index, U, lambda, traj_x, traj_u, fail_count, stats, stream, before, after);
    if (rc) return rc;
    return bounded_sync(h, s, who.c_str());
}

extern "C" int mpc_closed_loop_traffic(mpc_handle *h, int B, int T, int shift, int G, const double *radius, double reach,
                                       double *x, const double *cl, const int32_t *cl_index, double *U, double *lambda,
                                       double *table, double *traj_x, double *traj_u, int32_t *traj_opp, double *traj_clear,
                                       int32_t *fail_count, double *stats, void *stream)
{
    const std::string who = "mpc_closed_loop_traffic";
    int rc = check_scene_args(who, B, G, reach, radius); if (rc) return rc;
    if (T < 0) return fail(MPC_E_ARG, who + ": negative T");
    rc = check_common(h, B, who.c_str()); if (rc) return rc;
    if (h->cfg.constr_mode != MPC_CONSTR_DISCS) return fail(MPC_E_ARG, who + ": the handle's constr_mode is not MPC_CONSTR_DISCS");
    return closed_loop_traffic_impl(who, TAB_DISCS, h, B, T, shift, G, radius, reach, x, cl, cl_index, U, lambda, table, traj_x, traj_u,
                                    traj_opp, traj_clear, fail_count, stats, stream, [&](const double *X, const int32_t *opp) {
                                        return mpc_discs_from_plans(h, B, X, opp, radius, table, stream);
                                    });
}

extern "C" int mpc_closed_loop_traffic_field(mpc_handle *h, int B, int T, int shift, int G, const double *radius, const double *shape,
                                             double reach, double *x, const double *cl, const int32_t *cl_index, double *U,
                                             double *lambda, double *table, double *traj_x, double *traj_u, int32_t *traj_opp,
                                             double *traj_clear, int32_t *fail_count, double *stats, void *stream)
{
    const std::string who = "mpc_closed_loop_traffic_field";
    int rc = check_scene_args(who, B, G, reach, radius); if (rc) return rc;
    if (T < 0) return fail(MPC_E_ARG, who + ": negative T");
    if (!shape) return fail(MPC_E_ARG, who + ": null shape");
    rc = check_common(h, B, who.c_str()); if (rc) return rc;
    if (h->cfg.constr_mode == MPC_CONSTR_DISCS)
        return fail(MPC_E_ARG, who + ": the handle's constr_mode is MPC_CONSTR_DISCS: there an obstacle is a disc (mpc_closed_loop_traffic)");
    return closed_loop_traffic_impl(who, TAB_FIELDS, h, B, T, shift, G, radius, reach, x, cl, cl_index, U, lambda, table, traj_x, traj_u,
                                    traj_opp, traj_clear, fail_count, stats, stream, [&](const double *X, const int32_t *opp) {
                                        return mpc_fields_from_plans(h, B, X, opp, shape, table, stream);
                                    });
}

// ---------------------------------------------------------------------------------- scripted obstacles (mpc_obstacles.hpp)
static_assert(MPC_NDISC == MPC_NFIELD, "one sel [B][2] of mpc_obstacles_select serves the disc and the field table");
// what the four entry points ask of the scene and the tracks (checked without a device) ...
static int check_obstacle_args(const std::string &who, int B, int G, int K, int Lt, int ti, const char *ti_name, const void *obs)
{
    if (G < 1 || G > MPC_SCENE_MAX) return fail(MPC_E_ARG, who + ": the scene size G must be in [1, " + std::to_string(MPC_SCENE_MAX) + "]");
    if (K < 1 || K > MPC_SCENE_MAX) return fail(MPC_E_ARG, who + ": the number of obstacles K of a scene must be in [1, " + std::to_string(MPC_SCENE_MAX) + "]");
    if (B < 0) return fail(MPC_E_ARG, who + ": negative batch");
    if (B % G) return fail(MPC_E_ARG, who + ": the batch of " + std::to_string(B) + " agents is not a whole number of scenes of G = " +
                                       std::to_string(G) + " (B % G != 0: pad the scenes)");
    if (Lt < 1) return fail(MPC_E_ARG, who + ": Lt must be >= 1 samples per obstacle");
    if (ti < 0) return fail(MPC_E_ARG, who + ": " + ti_name + " must be >= 0");
    if (!obs) return fail(MPC_E_ARG, who + ": null obs");
    return MPC_OK;
}
// ... and of the window of `stages` samples from `ti` on: the kernels index it with an int
static int check_obstacle_window(const std::string &who, int ti, long long stages, const char *ti_name)
{
    if (ti + stages > 2147483647ll) return fail(MPC_E_ARG, who + ": " + ti_name + " plus the stages of the window does not fit an int32");
    return MPC_OK;
}
// W of the handle's obstacle samples: a disc on a handle of MPC_CONSTR_DISCS, a whole risk source on every other
static bool obstacle_discs(const mpc_handle *h) { return h->cfg.constr_mode == MPC_CONSTR_DISCS; }

// the selection on plans X [B][Nst][nx] against the window from sample `ti` (see obstacles_kernel for the three outputs)
// (held != null: the held form -- agent b compares the stages a plan of Nst of which held[b] are applied still holds)
static void launch_obstacles(mpc_handle *h, hipStream_t s, int B, int G, int K, int Lt, int wrap, int ti, int Nst, const double *X,
                             const double *obs, double reach, int32_t *sel, int32_t *sel_rec, size_t rec_stride, double *clear,
                             size_t clear_stride, int clear_slots, const int32_t *held = nullptr)
{
    int Gp = 1, Kp = 1;
    while (Gp < G) Gp <<= 1;
    while (Kp < K) Kp <<= 1;
    const int spw = 64 / std::max(Gp, Kp), scenes = B / G;
    const dim3 grid((unsigned)((scenes + spw - 1) / spw));
    with_flag(obstacle_discs(h), [&](auto DISCS) {
        if (held)
            hipLaunchKernelGGL((obstacles_kernel<DISCS() ? 3 : MPC_NFSRC, true, const int32_t *>), grid, dim3(TR_BLK), 0, s, B, G, K, Kp, spw,
                               Lt, wrap ? 1 : 0, ti, Nst, h->dc.nx, X, obs, reach * reach, sel, sel_rec, rec_stride, clear, clear_stride,
                               clear_slots, held);
        else
            hipLaunchKernelGGL((obstacles_kernel<DISCS() ? 3 : MPC_NFSRC>), grid, dim3(TR_BLK), 0, s, B, G, K, Kp, spw, Lt, wrap ? 1 : 0, ti,
                               Nst, h->dc.nx, X, obs, reach * reach, sel, sel_rec, rec_stride, clear, clear_stride, clear_slots);
    });
}

extern "C" int mpc_obstacles_select(mpc_handle *h, int B, int G, int K, int Lt, int wrap, int ti, int Nst, const double *X,
                                    const double *obs, double reach, int32_t *sel, double *clear, void *stream)
{
    const std::string who = "mpc_obstacles_select";
    if (Nst < 1) return fail(MPC_E_ARG, who + ": Nst must be >= 1 stages");
    int rc = check_obstacle_args(who, B, G, K, Lt, ti, "ti", obs); if (rc) return rc;
    rc = check_obstacle_window(who, ti, Nst, "ti"); if (rc) return rc;
    if (!(reach >= 0.0)) return fail(MPC_E_ARG, who + ": reach must be >= 0 (+inf: every obstacle of the scene)");
    if (!X || !sel) return fail(MPC_E_ARG, who + ": null X or sel");
    rc = check_common(h, B, who.c_str()); if (rc) return rc;
    rc = check_tables(h, B, who.c_str(), READS_ALL); if (rc) return rc;
    if (B == 0) return MPC_OK;
    launch_obstacles(h, (hipStream_t)stream, B, G, K, Lt, wrap, ti, Nst, X, obs, reach, sel, nullptr, 0, clear, MPC_NDISC, MPC_NDISC);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

// the gather of the window of the selected tracks from sample `ti` into table [B][N][MPC_NDISC][W] (rows_from_obstacles_kernel)
// (mask != null: the masked form -- the rows of the agents with mask[b] != 0 alone, and sel_plan[b] <- sel[b] for them)
static void launch_rows(mpc_handle *h, hipStream_t s, int B, int G, int K, int Lt, int wrap, int ti, const double *obs,
                        const int32_t *sel, double *table, const int32_t *mask = nullptr, int32_t *sel_plan = nullptr)
{
    const size_t words = (size_t)B * h->cfg.N * MPC_NDISC;
    const dim3 grid((unsigned)((words + 255) / 256));
    with_flag(obstacle_discs(h), [&](auto DISCS) {
        if (mask)
            hipLaunchKernelGGL((rows_from_obstacles_kernel<DISCS() ? 3 : MPC_NFSRC, true, RowMask>), grid, dim3(256), 0, s, B, h->cfg.N, G, K,
                               Lt, wrap ? 1 : 0, ti, obs, sel, table, RowMask{mask, sel_plan});
        else
            hipLaunchKernelGGL((rows_from_obstacles_kernel<DISCS() ? 3 : MPC_NFSRC>), grid, dim3(256), 0, s, B, h->cfg.N, G, K, Lt,
                               wrap ? 1 : 0, ti, obs, sel, table);
    });
}
// what the two public gathers check (`discs`: the disc form), asynchronous
static int rows_from_obstacles(const std::string &who, bool discs, mpc_handle *h, int B, int G, int K, int Lt, int wrap, int ti,
                               const double *obs, const int32_t *sel, double *table, void *stream)
{
    int rc = check_obstacle_args(who, B, G, K, Lt, ti, "ti", obs); if (rc) return rc;
    if (!sel || !table) return fail(MPC_E_ARG, who + ": null sel or table");
    rc = check_common(h, B, who.c_str()); if (rc) return rc;
    rc = check_obstacle_window(who, ti, h->cfg.N, "ti"); if (rc) return rc;
    if (discs && !obstacle_discs(h)) return fail(MPC_E_ARG, who + ": the handle's constr_mode is not MPC_CONSTR_DISCS");
    if (!discs && obstacle_discs(h))
        return fail(MPC_E_ARG, who + ": the handle's constraints are keep-out discs (constr_mode MPC_CONSTR_DISCS): there an obstacle is a disc "
                               "(mpc_set_agent_discs)");
    rc = check_tables(h, B, who.c_str(), READS_ALL); if (rc) return rc;
    if (B == 0) return MPC_OK;
    launch_rows(h, (hipStream_t)stream, B, G, K, Lt, wrap, ti, obs, sel, table);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}
extern "C" int mpc_discs_from_obstacles(mpc_handle *h, int B, int G, int K, int Lt, int wrap, int ti, const double *obs,
                                        const int32_t *sel, double *table, void *stream)
{
    return rows_from_obstacles("mpc_discs_from_obstacles", true, h, B, G, K, Lt, wrap, ti, obs, sel, table, stream);
}
extern "C" int mpc_fields_from_obstacles(mpc_handle *h, int B, int G, int K, int Lt, int wrap, int ti, const double *obs,
                                         const int32_t *sel, double *table, void *stream)
{
    return rows_from_obstacles("mpc_fields_from_obstacles", false, h, B, G, K, Lt, wrap, ti, obs, sel, table, stream);
}

// Road rows in time: row b of table [B][N][MPC_NROAD] = the window of N samples from `ti` of script row sidx[b]
// (roads_from_script_kernel), asynchronous.  The bound road table may be the target.
extern "C" int mpc_roads_from_script(mpc_handle *h, int B, int Lt, int wrap, int ti, const double *script, const int32_t *sidx,
                                     double *table, void *stream)
{
    const std::string who = "mpc_roads_from_script";
    if (B < 0) return fail(MPC_E_ARG, who + ": negative batch");
    if (Lt < 1) return fail(MPC_E_ARG, who + ": Lt must be >= 1 samples per script row");
    if (ti < 0) return fail(MPC_E_ARG, who + ": ti must be >= 0");
    if (!script || !sidx || !table) return fail(MPC_E_ARG, who + ": null script, sidx or table");
    int rc = check_common(h, B, who.c_str()); if (rc) return rc;
    rc = check_obstacle_window(who, ti, h->cfg.N, "ti"); if (rc) return rc;
    rc = check_tables(h, B, who.c_str(), READS_ALL); if (rc) return rc;
    if (B == 0) return MPC_OK;
    const size_t words = (size_t)B * h->cfg.N;
    hipLaunchKernelGGL(roads_from_script_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B, h->cfg.N, Lt,
                       wrap ? 1 : 0, ti, script, sidx, table);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

// Closed loop among scripted obstacles: per step (with a track) everybody's window of the track, everybody's plans
// (mpc_rollout), the nearest obstacle tracks of every agent's scene on them at the script's time t0 + t + 1, their window
// into the bound disc or field table, the solve, the plant step of mpc_closed_loop, and the clearance realised on the new
// states.  Every step is what the public call of that name launches; control returns to the host inside the solve alone.
// The step itself is plant_loop's, as in mpc_closed_loop and the traffic loops: this loop is its prologue and what it
// launches before the solve and behind the plant step.
extern "C" int mpc_closed_loop_obstacles(mpc_handle *h, int B, int T, int shift, int G, int K, int Lt, int wrap, int t0,
                                         const double *obs, double reach, double *x, const double *cl, int32_t *cl_index,
                                         double *U, double *lambda, double *table, double *traj_x, double *traj_u,
                                         int32_t *traj_sel, double *traj_clear, int32_t *fail_count, double *stats, void *stream,
                                         const mpc_track *trk)
{
    const std::string who = "mpc_closed_loop_obstacles";
    if (T < 0) return fail(MPC_E_ARG, who + ": negative T");
    int rc = check_obstacle_args(who, B, G, K, Lt, t0, "t0", obs); if (rc) return rc;
    if (!(reach >= 0.0)) return fail(MPC_E_ARG, who + ": reach must be >= 0 (+inf: every obstacle of the scene)");
    rc = check_common(h, B, who.c_str()); if (rc) return rc;
    rc = check_obstacle_window(who, t0, (long long)T + h->cfg.N, "t0"); if (rc) return rc;   // up to the last step's window
    if (trk) { rc = check_track(h, trk, who.c_str()); if (rc) return rc; }
    rc = check_tables(h, B, who.c_str(), READS_ALL, true); if (rc) return rc;
    rc = check_rewritten_table(h, obstacle_discs(h) ? TAB_DISCS : TAB_FIELDS, table, B, who); if (rc) return rc;
    rc = check_rate_rows(h, B, who); if (rc) return rc;
    if (B == 0 || T == 0) return MPC_OK;
    if (!x || !cl || !U || (h->dc.m && !lambda) || (trk && !cl_index)) return fail(MPC_E_ARG, who + ": null buffer");
    rc = reserve_traffic(h, B); if (rc) return rc;
    const int N = h->dc.N;
    TrafficBufs &tr = h->tr;
    hipStream_t s = (hipStream_t)stream;
    const auto before = [&](int t) -> int {
        const int ti = t0 + t + 1;   // the script's time of step t (and in `after`)
        if (trk) { const int rs = mpc_track_select(h, trk, B, x, cl, nullptr, cl_index, nullptr, stream); if (rs) return rs; }
        const int rr = mpc_rollout(h, B, N, x, U, tr.X, stream); if (rr) return rr;
        launch_obstacles(h, s, B, G, K, Lt, wrap, ti, N, tr.X, obs, reach, tr.opp, traj_sel ? traj_sel + (size_t)t * MPC_NDISC : nullptr,
                         (size_t)T * MPC_NDISC, nullptr, 0, 0);
        launch_rows(h, s, B, G, K, Lt, wrap, ti, obs, tr.opp, table);
        return MPC_OK;
    };
    const auto after = [&](int t) -> int {
        if (traj_clear)
            launch_obstacles(h, s, B, G, K, Lt, wrap, t0 + t + 1, 1, x, obs, INFINITY, nullptr, nullptr, 0, traj_clear + t, (size_t)T, 1);
        return MPC_OK;
    };
    rc = plant_loop(h, B, T, shift, x, cl, cl_index, U, lambda, traj_x, traj_u, fail_count, stats, stream, before, after);
    if (rc) return rc;
    return bounded_sync(h, s, who.c_str());
}

// ------------------------------------------------------------------- event-triggered holding among scripted obstacles
// what mpc_obstacle_trigger and mpc_closed_loop_obstacles_event ask of the rule's arguments (checked without a device)
static int check_obstacle_rule(const std::string &who, double reach, double clear_thr, int watch)
{
    if (!(reach >= 0.0)) return fail(MPC_E_ARG, who + ": reach must be >= 0 (+inf: every obstacle of the scene)");
    if (!(clear_thr <= reach * reach))
        return fail(MPC_E_ARG, who + ": clear_thr must be a number <= reach^2 (the selection sees no clearance beyond reach)");
    if (watch < 0 || watch > 3) return fail(MPC_E_ARG, who + ": watch must be in [0, 3] (bit 0: the clearance rule, bit 1: the new-obstacle rule)");
    return MPC_OK;
}
// the selection over the stages every plan still holds, then the rule (sel_chk [B][MPC_NDISC], clear_chk [B][MPC_NDISC])
static void launch_obstacle_trigger(mpc_handle *h, hipStream_t s, int B, int G, int K, int Lt, int wrap, int ti, const double *X,
                                    const double *obs, double reach, const int32_t *held, const int32_t *sel_plan, double clear_thr,
                                    int watch, const int32_t *fire_in, int32_t *sel_chk, double *clear_chk, uint8_t *why,
                                    size_t why_stride, int32_t *fire_out)
{
    launch_obstacles(h, s, B, G, K, Lt, wrap, ti, h->cfg.N, X, obs, reach, sel_chk, nullptr, 0, clear_chk, MPC_NDISC, MPC_NDISC, held);
    hipLaunchKernelGGL(obstacle_rule_kernel, grid_for(B, 64), dim3(64), 0, s, B, held, sel_chk, clear_chk, sel_plan, clear_thr, watch,
                       fire_in, fire_out, why, why_stride);
}

extern "C" int mpc_obstacle_trigger(mpc_handle *h, int B, int G, int K, int Lt, int wrap, int ti, const double *X, const double *obs,
                                    double reach, const int32_t *held, const int32_t *sel_plan, double clear_thr, int watch,
                                    const int32_t *fire_in, int32_t *sel_chk, double *clear_chk, uint8_t *why, int32_t *fire_out,
                                    void *stream)
{
    const std::string who = "mpc_obstacle_trigger";
    int rc = check_obstacle_args(who, B, G, K, Lt, ti, "ti", obs); if (rc) return rc;
    rc = check_obstacle_rule(who, reach, clear_thr, watch); if (rc) return rc;
    if (!X || !held || !sel_plan || !sel_chk || !clear_chk || !fire_out)
        return fail(MPC_E_ARG, who + ": null X, held, sel_plan, sel_chk, clear_chk or fire_out");
    rc = check_common(h, B, who.c_str()); if (rc) return rc;
    rc = check_obstacle_window(who, ti, h->cfg.N, "ti"); if (rc) return rc;
    rc = check_tables(h, B, who.c_str(), READS_ALL); if (rc) return rc;
    if (B == 0) return MPC_OK;
    launch_obstacle_trigger(h, (hipStream_t)stream, B, G, K, Lt, wrap, ti, X, obs, reach, held, sel_plan, clear_thr, watch, fire_in,
                            sel_chk, clear_chk, why, 1, fire_out);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

// The event-triggered loop among scripted obstacles: closed_loop_event_impl with the hook of the obstacles -- every launch
// the one the public call of that name makes (see include/mpc_hip.h for the eleven steps)
struct ObstacleEventHook {
    static constexpr bool on = true;
    mpc_handle *h; hipStream_t s; void *stream;
    int B, T, shift, G, K, Lt, wrap, t0;
    const double *obs; double reach, clear_thr; int watch;
    double *x, *U; int32_t *held, *sel_plan; double *table;
    int32_t *traj_sel; double *traj_clear; uint8_t *traj_why;
    // steps 2 - 4: what every agent will go on applying, the rule on top of `fire`, the shift of the agents that fire
    int fired(int t, int32_t *fire) const
    {
        const int rr = mpc_rollout_held(h, B, x, U, held, h->tr.X, stream); if (rr) return rr;
        launch_obstacle_trigger(h, s, B, G, K, Lt, wrap, t0 + t + 1, h->tr.X, obs, reach, held, sel_plan, clear_thr, watch, fire,
                                h->orule.sel_chk, h->orule.clear_chk, traj_why ? traj_why + t : nullptr, (size_t)T, fire);
        if (shift) hipLaunchKernelGGL(plan_shift_kernel, grid_for(B, 64), dim3(64), 0, s, B, h->dc.N, held, fire, U);
        return MPC_OK;
    }
    // steps 6 - 7: everybody's selection on the full window, the rows and sel_plan of the agents that fire
    int selected(int t, int32_t *fire) const
    {
        const int ti = t0 + t + 1;
        launch_obstacles(h, s, B, G, K, Lt, wrap, ti, h->dc.N, h->tr.X, obs, reach, h->tr.opp,
                         traj_sel ? traj_sel + (size_t)t * MPC_NDISC : nullptr, (size_t)T * MPC_NDISC, nullptr, 0, 0);
        launch_rows(h, s, B, G, K, Lt, wrap, ti, obs, h->tr.opp, table, fire, sel_plan);
        return MPC_OK;
    }
    // step 11: the realised clearance on the new states
    int stepped(int t, int32_t *) const
    {
        if (traj_clear)
            launch_obstacles(h, s, B, G, K, Lt, wrap, t0 + t + 1, 1, x, obs, INFINITY, nullptr, nullptr, 0, traj_clear + t, (size_t)T, 1);
        return MPC_OK;
    }
};
extern "C" int mpc_closed_loop_obstacles_event(mpc_handle *h, int B, int T, int shift, const double *w, double thr, int max_hold, int G,
                                               int K, int Lt, int wrap, int t0, const double *obs, double reach, double clear_thr,
                                               int watch, double *x, const double *cl, int32_t *cl_index, double *U, double *lambda,
                                               int32_t *held, int32_t *sel_plan, double *table, const double *disturbance,
                                               double *traj_x, double *traj_u, int32_t *traj_sel, double *traj_clear,
                                               uint8_t *traj_why, uint8_t *solved, int32_t *solve_count, int32_t *fail_count,
                                               double *stats, void *stream, const mpc_track *trk)
{
    const char *who_ = "mpc_closed_loop_obstacles_event";
    const std::string who(who_);
    int rc = check_trigger_args(who_, w, thr, max_hold, held); if (rc) return rc;
    if (T < 0) return fail(MPC_E_ARG, who + ": negative T");
    rc = check_obstacle_args(who, B, G, K, Lt, t0, "t0", obs); if (rc) return rc;
    rc = check_obstacle_rule(who, reach, clear_thr, watch); if (rc) return rc;
    if (!sel_plan) return fail(MPC_E_ARG, who + ": null sel_plan");
    if (!h) return fail(MPC_E_ARG, who + ": null handle");
    rc = check_max_hold(h, who_, max_hold); if (rc) return rc;
    rc = check_common(h, B, who_); if (rc) return rc;
    rc = check_obstacle_window(who, t0, (long long)T + h->cfg.N, "t0"); if (rc) return rc;   // up to the last step's window
    if (trk) { rc = check_track(h, trk, who_); if (rc) return rc; }
    rc = check_tables(h, B, who_, READS_ALL, true); if (rc) return rc;
    rc = check_rewritten_table(h, obstacle_discs(h) ? TAB_DISCS : TAB_FIELDS, table, B, who); if (rc) return rc;
    rc = check_rate_rows(h, B, who); if (rc) return rc;
    if (B == 0 || T == 0) return MPC_OK;
    // every refusal stands before the first allocation (closed_loop_event_impl repeats the ones it shares)
    if (!x || !cl || !U || (h->dc.m && !lambda) || (trk && !cl_index)) return fail(MPC_E_ARG, who + ": null buffer");
    rc = reserve_traffic(h, B); if (rc) return rc;
    rc = reserve_obstacle_rule(h, B); if (rc) return rc;
    const ObstacleEventHook hook{h, (hipStream_t)stream, stream, B, T, shift, G, K, Lt, wrap, t0, obs, reach, clear_thr, watch,
                                 x, U, held, sel_plan, table, traj_sel, traj_clear, traj_why};
    return closed_loop_event_impl(who_, h, B, T, shift, w, thr, max_hold, x, cl, cl_index, U, lambda, held, disturbance, traj_x, traj_u,
                                  solved, solve_count, fail_count, stats, stream, trk, cl_index, nullptr, hook);
}

// ------------------------------------------------------------------------------ event-triggered holding in traffic
// the selection of opponents over the stages every plan still holds, then the rule of the obstacles on global agent
// indices (opp_chk [B][MPC_NDISC], clear_chk [B][MPC_NDISC])
static void launch_opponent_trigger(mpc_handle *h, hipStream_t s, int B, int G, const double *X, const double *radius, double reach,
                                    const int32_t *held, const int32_t *opp_plan, double clear_thr, int watch, const int32_t *fire_in,
                                    int32_t *opp_chk, double *clear_chk, uint8_t *why, size_t why_stride, int32_t *fire_out)
{
    launch_opponents(h, s, B, G, h->cfg.N, X, radius, reach, opp_chk, nullptr, 0, clear_chk, MPC_NDISC, MPC_NDISC, held);
    hipLaunchKernelGGL(obstacle_rule_kernel, grid_for(B, 64), dim3(64), 0, s, B, held, opp_chk, clear_chk, opp_plan, clear_thr, watch,
                       fire_in, fire_out, why, why_stride);
}

extern "C" int mpc_opponent_trigger(mpc_handle *h, int B, int G, const double *X, const double *radius, double reach,
                                    const int32_t *held, const int32_t *opp_plan, double clear_thr, int watch,
                                    const int32_t *fire_in, int32_t *opp_chk, double *clear_chk, uint8_t *why, int32_t *fire_out,
                                    void *stream)
{
    const std::string who = "mpc_opponent_trigger";
    int rc = check_scene_args(who, B, G, reach, radius); if (rc) return rc;
    rc = check_obstacle_rule(who, reach, clear_thr, watch); if (rc) return rc;
    if (!X || !held || !opp_plan || !opp_chk || !clear_chk || !fire_out)
        return fail(MPC_E_ARG, who + ": null X, held, opp_plan, opp_chk, clear_chk or fire_out");
    rc = check_common(h, B, who.c_str()); if (rc) return rc;
    rc = check_tables(h, B, who.c_str(), READS_ALL); if (rc) return rc;
    if (B == 0) return MPC_OK;
    launch_opponent_trigger(h, (hipStream_t)stream, B, G, X, radius, reach, held, opp_plan, clear_thr, watch, fire_in, opp_chk,
                            clear_chk, why, 1, fire_out);
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

// the gather of the selected opponents' plans into the rows of the agents with mask[b] != 0 alone, and opp_plan[b] <- opp[b]
// for them (the masked forms of discs_from_plans_kernel / fields_from_plans_kernel; `per`: radius [B] or shape [B][4])
static void launch_plan_rows_masked(mpc_handle *h, hipStream_t s, bool discs, int B, const double *X, const int32_t *opp, const double *per,
                                    double *table, const int32_t *mask, int32_t *opp_plan)
{
    const size_t words = (size_t)B * h->cfg.N * MPC_NDISC;   // (== MPC_NFIELD)
    const dim3 grid((unsigned)((words + 255) / 256));
    if (discs)
        hipLaunchKernelGGL((discs_from_plans_kernel<true, RowMask>), grid, dim3(256), 0, s, B, h->cfg.N, h->dc.nx, X, opp, per, table,
                           RowMask{mask, opp_plan});
    else
        hipLaunchKernelGGL((fields_from_plans_kernel<true, RowMask>), grid, dim3(256), 0, s, B, h->cfg.N, h->dc.nx, X, opp, per, table,
                           RowMask{mask, opp_plan});
}

// The event-triggered traffic loop: closed_loop_event_impl with the hook of the traffic -- every launch the one the public
// call of that name makes (see include/mpc_hip.h for the ten steps)
struct TrafficEventHook {
    static constexpr bool on = true;
    mpc_handle *h; hipStream_t s; void *stream;
    int B, T, shift, G;
    const double *radius, *per; bool discs; double reach, clear_thr; int watch;
    double *x, *U; int32_t *held, *opp_plan; double *table;
    int32_t *traj_opp; double *traj_clear; uint8_t *traj_why;
    // steps 2 - 4: what every agent will go on applying, the rule on top of `fire`, the shift of the agents that fire
    int fired(int t, int32_t *fire) const
    {
        const int rr = mpc_rollout_held(h, B, x, U, held, h->tr.X, stream); if (rr) return rr;
        launch_opponent_trigger(h, s, B, G, h->tr.X, radius, reach, held, opp_plan, clear_thr, watch, fire, h->orule.sel_chk,
                                h->orule.clear_chk, traj_why ? traj_why + t : nullptr, (size_t)T, fire);
        if (shift) hipLaunchKernelGGL(plan_shift_kernel, grid_for(B, 64), dim3(64), 0, s, B, h->dc.N, held, fire, U);
        return MPC_OK;
    }
    // steps 5 - 6: everybody's selection on the full horizon, the rows and opp_plan of the agents that fire
    int selected(int t, int32_t *fire) const
    {
        launch_opponents(h, s, B, G, h->dc.N, h->tr.X, radius, reach, h->tr.opp, traj_opp ? traj_opp + (size_t)t * MPC_NDISC : nullptr,
                         (size_t)T * MPC_NDISC, nullptr, 0, 0);
        launch_plan_rows_masked(h, s, discs, B, h->tr.X, h->tr.opp, per, table, fire, opp_plan);
        return MPC_OK;
    }
    // step 10: the realised clearance on the new states
    int stepped(int t, int32_t *) const
    {
        if (traj_clear) launch_opponents(h, s, B, G, 1, x, radius, INFINITY, nullptr, nullptr, 0, traj_clear + t, (size_t)T, 1);
        return MPC_OK;
    }
};
extern "C" int mpc_closed_loop_traffic_event(mpc_handle *h, int B, int T, int shift, const double *w, double thr, int max_hold, int G,
                                             const double *radius, const double *shape, double reach, double clear_thr, int watch,
                                             double *x, const double *cl, const int32_t *cl_index, double *U, double *lambda,
                                             int32_t *held, int32_t *opp_plan, double *table, const double *disturbance,
                                             double *traj_x, double *traj_u, int32_t *traj_opp, double *traj_clear,
                                             uint8_t *traj_why, uint8_t *solved, int32_t *solve_count, int32_t *fail_count,
                                             double *stats, void *stream)
{
    const char *who_ = "mpc_closed_loop_traffic_event";
    const std::string who(who_);
    int rc = check_trigger_args(who_, w, thr, max_hold, held); if (rc) return rc;
    if (T < 0) return fail(MPC_E_ARG, who + ": negative T");
    rc = check_scene_args(who, B, G, reach, radius); if (rc) return rc;
    rc = check_obstacle_rule(who, reach, clear_thr, watch); if (rc) return rc;
    if (!opp_plan) return fail(MPC_E_ARG, who + ": null opp_plan");
    if (!h) return fail(MPC_E_ARG, who + ": null handle");
    rc = check_max_hold(h, who_, max_hold); if (rc) return rc;
    rc = check_common(h, B, who_); if (rc) return rc;
    const bool discs = obstacle_discs(h);
    if (discs && shape)
        return fail(MPC_E_ARG, who + ": the handle's constr_mode is MPC_CONSTR_DISCS: there an opponent is a disc and shape must be NULL");
    if (!discs && !shape) return fail(MPC_E_ARG, who + ": null shape (the handle's opponents are risk fields: shape [B][4])");
    rc = check_tables(h, B, who_, READS_ALL, true); if (rc) return rc;
    rc = check_rewritten_table(h, discs ? TAB_DISCS : TAB_FIELDS, table, B, who); if (rc) return rc;
    rc = check_rate_rows(h, B, who); if (rc) return rc;
    if (B == 0 || T == 0) return MPC_OK;
    // every refusal stands before the first allocation (closed_loop_event_impl repeats the ones it shares)
    if (!x || !cl || !U || (h->dc.m && !lambda)) return fail(MPC_E_ARG, who + ": null buffer");
    rc = reserve_traffic(h, B); if (rc) return rc;
    rc = reserve_obstacle_rule(h, B); if (rc) return rc;
    const TrafficEventHook hook{h, (hipStream_t)stream, stream, B, T, shift, G, radius, discs ? radius : shape, discs, reach, clear_thr,
                                watch, x, U, held, opp_plan, table, traj_opp, traj_clear, traj_why};
    return closed_loop_event_impl(who_, h, B, T, shift, w, thr, max_hold, x, cl, cl_index, U, lambda, held, disturbance, traj_x, traj_u,
                                  solved, solve_count, fail_count, stats, stream, nullptr, nullptr, nullptr, hook);
}

extern "C" int mpc_last_speculation(mpc_handle *h, int64_t *issued, int64_t *used)
{
    { const int rb = refuse_if_busy(h, "mpc_last_speculation"); if (rb) return rb; }
    if (issued) *issued = h->spec_issued;
    if (used) *used = h->spec_used;
    return MPC_OK;
}

extern "C" int mpc_last_lookahead(mpc_handle *h, int64_t *evals, int64_t *hits)
{
    { const int rb = refuse_if_busy(h, "mpc_last_lookahead"); if (rb) return rb; }
    if (evals) *evals = h->la_evals;
    if (hits) *hits = h->la_hits;
    return MPC_OK;
}

extern "C" int mpc_last_solve_info2(mpc_handle *h, double *launch_pairs, int64_t *lbfgs_rows)
{
    { const int rb = refuse_if_busy(h, "mpc_last_solve_info2"); if (rb) return rb; }
    if (launch_pairs) *launch_pairs = (double)h->launches; // (step, eval) launch sets of the last solve
    if (lbfgs_rows) *lbfgs_rows = h->lbfgs_rows;
    return MPC_OK;
}

extern "C" int mpc_last_solve_info(mpc_handle *h, int64_t *rounds, int64_t *evals_grad, int64_t *evals_cost,
                                   double *eval_ms, double *step_ms)
{
    { const int rb = refuse_if_busy(h, "mpc_last_solve_info"); if (rb) return rb; }
    if (rounds) *rounds = h->rounds;
    if (evals_grad) *evals_grad = h->evals_grad;
    if (evals_cost) *evals_cost = h->evals_cost;
    if (eval_ms) *eval_ms = h->eval_ms;
    if (step_ms) *step_ms = h->step_ms;
    return MPC_OK;
}

extern "C" int mpc_last_kernel_ms(mpc_handle *h, double *out4)
{
    if (!h || !out4) return fail(MPC_E_ARG, "mpc_last_kernel_ms: null argument");
    { const int rb = refuse_if_busy(h, "mpc_last_kernel_ms"); if (rb) return rb; }
    for (int k = 0; k < 4; k++) out4[k] = h->kernel_ms[k];
    return MPC_OK;
}

extern "C" int mpc_last_kernel_profile(mpc_handle *h, double *ms5, int64_t *launches5, int64_t *solo_agents)
{
    { const int rb = refuse_if_busy(h, "mpc_last_kernel_profile"); if (rb) return rb; }
    for (int k = 0; k < 5; k++) {
        if (ms5) ms5[k] = h->kernel_ms[k];
        if (launches5) launches5[k] = h->kernel_launches[k];
    }
    if (solo_agents) *solo_agents = h->solo_agents;
    return MPC_OK;
}

extern "C" int mpc_set_nearest_blocks(mpc_handle *h, int on)
{
    { const int rb = refuse_if_busy(h, "mpc_set_nearest_blocks"); if (rb) return rb; }
    if (on == 1) return fail(MPC_E_ARG, "mpc_set_nearest_blocks: mode 1 (the block-box search) was removed: 0 (full scan) or 2 (grid)");
    if (on != 0 && on != 2) return fail(MPC_E_ARG, "mpc_set_nearest_blocks: mode is 0 (full scan) or 2 (grid)");
    h->nearest_mode = on;
    return MPC_OK;
}

extern "C" int mpc_set_solo_max(mpc_handle *h, int max_requests)
{
    if (!h || max_requests < 0) return fail(MPC_E_ARG, "mpc_set_solo_max: bad argument");
    { const int rb = refuse_if_busy(h, "mpc_set_solo_max"); if (rb) return rb; }
    h->solo_max = h->solo_all = max_requests;
    return MPC_OK;
}

extern "C" int mpc_last_solo_ms(mpc_handle *h, double *sum_ms, double *longest_ms)
{
    { const int rb = refuse_if_busy(h, "mpc_last_solo_ms"); if (rb) return rb; }
    if (sum_ms) *sum_ms = h->kernel_ms[4];
    if (longest_ms) *longest_ms = h->solo_longest_ms;
    return MPC_OK;
}

extern "C" int mpc_stream_concurrency(mpc_handle *h, int *streams, int *groups_last)
{
    { const int rb = refuse_if_busy(h, "mpc_stream_concurrency"); if (rb) return rb; }
    if (streams) *streams = h->hw_queues;
    if (groups_last) *groups_last = h->groups_last;
    return MPC_OK;
}

extern "C" int mpc_set_round_limit(mpc_handle *h, int64_t rounds)
{
    if (!h || rounds < 0) return fail(MPC_E_ARG, "mpc_set_round_limit: bad argument");
    { const int rb = refuse_if_busy(h, "mpc_set_round_limit"); if (rb) return rb; }
    h->round_limit = (long long)rounds;
    return MPC_OK;
}

extern "C" int mpc_set_memo(mpc_handle *h, int on)
{
    { const int rb = refuse_if_busy(h, "mpc_set_memo"); if (rb) return rb; }
    h->dc.no_memo = on ? 0 : 1;
    return MPC_OK;
}

extern "C" int mpc_set_groups(mpc_handle *h, int groups)
{
    if (!h || groups < 0 || groups > MPC_MAX_GROUPS) return fail(MPC_E_ARG, "mpc_set_groups: bad argument");
    { const int rb = refuse_if_busy(h, "mpc_set_groups"); if (rb) return rb; }
    h->ngroups = groups;
    return MPC_OK;
}

extern "C" int mpc_set_profile(mpc_handle *h, int on)
{
    { const int rb = refuse_if_busy(h, "mpc_set_profile"); if (rb) return rb; }
    h->profile = on != 0;
    return MPC_OK;
}

extern "C" int mpc_set_poll_timeout(mpc_handle *h, double seconds)
{
    if (!h || !(seconds > 0.0)) return fail(MPC_E_ARG, "mpc_set_poll_timeout: bad argument");
    { const int rb = refuse_if_busy(h, "mpc_set_poll_timeout"); if (rb) return rb; }
    h->poll_timeout_s = seconds;
    return MPC_OK;
}

// test aid: the library's idling kernel (one wave that sleeps until `microseconds` of the device's wall clock have
// passed) queued on `stream` -- work that holds a stream for a known time (the wall-clock bound's test)
extern "C" int mpc_debug_spin(mpc_handle *h, double microseconds, void *stream)
{
    int rc = check_common(h, 0, "mpc_debug_spin"); if (rc) return rc;
    if (!(microseconds >= 0.0) || microseconds > 30e6) return fail(MPC_E_ARG, "mpc_debug_spin: 0 .. 30 s");
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device) != hipSuccess || khz <= 0) khz = 100000;
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long)(microseconds * 1e-6 * khz * 1e3));
    HIPCHK(hipGetLastError());
    return MPC_OK;
}

// diagnostic: the per-agent solver records as the last solve left them (after a solve stopped by max_total_inner = k
// they hold the state at the top of inner iteration k: step sizes, line-search step, active-set size, history
// fill, counters), decoded to plain doubles, into a HOST array [B][MPC_NREC]; names: mpc_debug_record_names()
static const char *const k_record_names =
    "psi,L,gamma,phi,psixh,pp,gp,tau,psin,Ln,gamman,psixhn,gpn,ppn,sigpp,eps,hn2,hfd,gamma_top,Delta,rho,eps_old,ne1,ps_eps,"
    "out_eps,out_delta,psi_out,psie,phase,k,lidx,lfull,noprog,nJ,outer,first,initred,penred,inner_tot,inner_fail,status,"
    "nevals,maxit,overwrite,fallback,ps_status,ps_iters,out_of_iter,ngrad,lbrows,spec,spec_gamma,nspec,nspec_used,ncost,"
    "run_mineps,run_ev0,memo_status,memo_iters,memo_evals,memo_mineps,memo_eps,la_evals,la_hits";
static_assert(R_USED == 64 && REC == MPC_NREC, "k_record_names / MPC_NREC must follow the record enum");
extern "C" const char *mpc_debug_record_names(void) { return k_record_names; }
extern "C" int mpc_debug_records(mpc_handle *h, int B, double *host_out)
{
    int rc = check_common(h, B, "mpc_debug_records"); if (rc) return rc;
    if (!host_out) return fail(MPC_E_ARG, "mpc_debug_records: null buffer");
    if (B == 0) return MPC_OK;
    if (!h->arena.p || B > h->ws.B) return fail(MPC_E_ARG, "mpc_debug_records: more agents than the last solve held");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(host_out, h->ws.rec, sizeof(double) * (size_t)B * REC, hipMemcpyDeviceToHost));
    for (int a = 0; a < B; a++)
        for (int sl = 0; sl < REC; sl++)
            if (rec_is_int(sl)) {
                int64_t bits; std::memcpy(&bits, &host_out[(size_t)a * REC + sl], 8);
                host_out[(size_t)a * REC + sl] = (double)(int32_t)(bits & 0xffffffffLL);
            }
    return MPC_OK;
}

#ifdef MPC_DEV_STAMP
extern "C" int mpc_dev_records(mpc_handle *h, double *host_out)   // (experiment) the per-agent records as the last solve left them
{
    (void)hipDeviceSynchronize();
    return hipMemcpy(host_out, h->ws.rec, sizeof(double) * (size_t)h->ws.B * mpc::REC, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
}
extern "C" int mpc_dev_stamps(long long *host_out)       // (timing experiment) the stamps of the last launch of the kernel chosen
{
    (void)hipDeviceSynchronize();
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(mpc::g_dev_stamps), sizeof(long long) * 4 * mpc::DEV_STAMPS) == hipSuccess ? 0 : 1;
}
#endif
