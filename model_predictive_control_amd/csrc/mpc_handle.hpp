// mpc_handle.hpp -- host side of libmpc_hip.so, part 1: the handle behind the C-ABI, its configuration check, environment
// switches, stream-concurrency probe, the reserve_* calls that grow its memory (owner and layouts: mpc_arena.hpp), bounded
// waits, and the per-agent tables bound to it (one BoundTable per TableKind, one batch-size check for all of them:
// check_tables).  Host code (plus the probe's idling kernel); included by mpc_api.hip alone.
#pragma once
#include "mpc_arena.hpp"
#include "mpc_aux.hpp"
#include "mpc_solo.hpp"
#include "mpc_game.hpp"
#include "mpc_traffic.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <array>
#include <vector>

#define MPC_GRID_MAX_ROWS 1024   // centerline rows the nearest-point grid is built for (256 KB each)

// the kinds of per-agent table (TableKind: mpc_arena.hpp) an entry point reads, as a mask
enum : unsigned { READS_PARAMS = 1u << TAB_PARAMS, READS_BOX = 1u << TAB_BOX, READS_CONSTR = 1u << TAB_CONSTR, READS_DISCS = 1u << TAB_DISCS,
                  READS_RATES = 1u << TAB_RATES, READS_FIELDS = 1u << TAB_FIELDS, READS_ROADS = 1u << TAB_ROADS, READS_ALL = (1u << TAB_KINDS) - 1 };
// messages, doubles per row (width_per_N: per stage of the handle's horizon -- table_width)
static constexpr struct { const char *noun, *setter; int width, width_per_N; } k_tables[TAB_KINDS] = {
    {"parameter", "mpc_set_agent_params", MPC_NPARAM, 0},
    {"bounds", "mpc_set_agent_bounds", MPC_NBOUND, 0},
    {"constraint", "mpc_set_agent_constraints", MPC_NCONSTR, 0},
    {"disc", "mpc_set_agent_discs", 0, 3 * MPC_NDISC},
    {"rate", "mpc_set_agent_rates", MPC_NRATE, 0},
    {"field", "mpc_set_agent_fields", 0, MPC_NFIELD * MPC_NFSRC},
    {"road", "mpc_set_agent_roads", 0, MPC_NROAD}};
struct BoundTable {
    const double *table = nullptr;         // [rows][k_tables[kind].width], null: none bound
    const int32_t *idx = nullptr;          // [B] the row per agent
    int rows = 0, B = 0;
};
// the row indices of the agents of one solve, per kind: the handle's bound ones, or a masked solve's gathered ones
struct AgentIdx { const int32_t *of[TAB_KINDS]; };

// The workspace as the host keeps it: the kernels' Workspace, the parameter table the per-agent kernels get with it
// (WorkspacePA: ptab / pidx, a kernel argument), and the caller's other tables by kind (null: none bound).  Each of those
// reaches the kernel forms that read it as an argument of its own -- the device struct its accessor returns -- and no other
// kernel at all (which forms those are: with_table_form and launch_step_t in mpc_launch.hpp).
struct WorkspaceHost : WorkspacePA {
    struct Tab {
        const double *table;                       // [P][table_width(kind)] caller's table
        const int *rows;                           // [B]                    caller's row index per agent
    } tabs[TAB_KINDS];                             // (tabs[TAB_PARAMS] stays null: ptab / pidx above)
    bool bound(TableKind k) const { return tabs[k].table != nullptr; }
    template <class T> T as(TableKind k) const { return T{tabs[k].table, tabs[k].rows}; }
    BoxTab box() const { return as<BoxTab>(TAB_BOX); }
    ConTab con() const { return as<ConTab>(TAB_CONSTR); }
    DiscTab disc() const { return as<DiscTab>(TAB_DISCS); }
    RateTab rate() const { return as<RateTab>(TAB_RATES); }
    FieldTab field() const { return as<FieldTab>(TAB_FIELDS); }
    RoadTab road() const { return as<RoadTab>(TAB_ROADS); }
};

struct mpc_handle {
    mpc_config cfg;
    DevCfg dc;
    int device = 0;
    int wide_max = 4096;        // requests per round up to which K1a runs one wave per request (MPC_WIDE_MAX)
    int apb_env = 0;            // MPC_APB: agents per step-kernel workgroup (4, 16, 64; 0 = by batch size)
    bool fused_eval = true;     // K1b + K1c in one launch (MPC_UNFUSED_EVAL: the two-kernel path)
    int fused_max = 1 << 30;    // ... while a round holds at most this many requests (MPC_FUSED_MAX).  Every round since the
                                // step kernel's workgroups hold 38 KB of LDS instead of 51 (round 3): the fused kernel's
                                // 44 KB workgroups now share a CU with them, and the stage records never leave LDS
                                // (rounds 1 - 2: 16384 -- beyond that the two-kernel path was faster)
    bool quad_rollout = true;   // K1a by two (kinematic) / four (Pacejka) lanes per request (MPC_NO_QUAD: one thread)
    int pac_quad_max = 24576;   // Pacejka: requests bound of a round up to which K1a runs four lanes per request (MPC_PAC_QUAD_MAX)
    bool step_regs = false;     // MPC_STEP_REGS: the two-loop reads the history from global memory, not from an LDS copy
    int chain_min = 24576;      // MPC_CHAIN_MIN: requests bound of a group's round from which the thread-per-agent blocks
                                // (chain_block) ride in its step launch.  Measured with the one-wave form (r03_experiments 18):
                                // 65 536 agents (groups of 16 384) +1.2 % with them; 32 768 agents (groups of 10 923)
                                // and 16 384 (groups of 8 192) -1 ... -2 %: only the full rounds of big groups
    int spec_depth = 1;         // MPC_SPEC_DEPTH: under MPC_SPEC_POLICY=2, the descent-lemma retry of a line-search trial from which
                                // no speculative gradient is issued in the launches that carry chain blocks (1 = every retry, 2 = from the second doubling on).
                                // Measured, 65 536 kinematic agents, alternating on one box (profiles/r16_speculation.txt): policy 0
                                // 498.9 - 500.9 k solves/s, policy 1 502.9 - 504.0 k, policy 2 at depth 2 503.2 - 505.2 k, at depth 1
                                // 505.6 - 507.6 k
    int lds_pairs = 0;          // MPC_LDS_PAIRS: history pairs the step kernel's LDS copy holds (0 = chosen by launch_step_t)
    int num_cus = 256;
    int nearest_mode = 2;                 // mpc_set_nearest_blocks: 0 full scan (MPC_NEAREST_SCAN), 2 grid of index ranges (default);
                                          // a table that mpc_centerline_blocks has not prepared takes the full scan
    const double *cl_grid_for = nullptr;             // the table `grid` was prepared for (device pointer identity), or null
    GridBufs grid;
    int solo_all = 4096;        // a batch of at most this many agents runs in the persistent kernel from the start
                                // (MPC_SOLO_ALL; measured: kinematic 4 096 agents 62.8 -> 53.3 ms, 8 192 worse; Pacejka 1 024)
    int solo_max = 1024;        // a group with at most this many requests per round finishes in the persistent
                                // wave-per-agent kernel (MPC_SOLO_MAX / mpc_set_solo_max; 0 = rounds only).
                                // Default 1024 (kinematic model, measured in round 2, also for N = 40: profiles/r02c_*),
                                // 128 on the Pacejka model (round 4: mpc_create)
    // Memory: every allocation is a DevBuf member of the handle (or of one of its *Bufs), freed with it; what is carved
    // out of one follows that arena's layout function (mpc_arena.hpp)
    int Bp_alloc = 0;      // workspace capacity (agents)
    DevBuf arena;          // carved into the Workspace arrays (workspace_layout)
    WorkspaceHost ws{};
    DevBuf pinned_mem{true};
    PinnedCounts &pinned() const { return *reinterpret_cast<PinnedCounts *>(pinned_mem.p); }
    hipEvent_t pollev[2][MPC_MAX_GROUPS] = {{nullptr}};
    hipEvent_t soloev[MPC_MAX_GROUPS][2] = {{nullptr}}; // profile mode: around a group's persistent-kernel launch
    // profiling of the last solve
    bool profile = false;
    int64_t rounds = 0, evals_grad = 0, evals_cost = 0, launches = 0;
    double eval_ms = 0.0, step_ms = 0.0, lbfgs_ms = 0.0;
    double kernel_ms[5] = {0, 0, 0, 0, 0}; // step, K1a rollout, K1b stage, K1c adjoint, solo (profile mode)
    int64_t kernel_launches[5] = {0, 0, 0, 0, 0};
    int64_t solo_agents = 0;    // agents finished by the persistent kernel in the last solve
    double solo_longest_ms = 0.0; // profile mode: the longest of the groups' persistent-kernel launches
    int64_t spec_issued = 0, spec_used = 0; // speculative channel-2 gradients of the last solve
    int64_t la_evals = 0, la_hits = 0;      // persistent kernel's lookahead: candidate evaluations executed, requests served from them
    int64_t lbfgs_rows = 0; // history pairs read by K3 (each is read twice: 4*n*8 bytes per pair)
    std::vector<hipEvent_t> ev_pool;
    // sub-batch pipelining: the batch is split into groups that run their rounds on separate
    // streams, so that one group's (latency-bound) solver step overlaps another group's evaluation
    // mpc_solve_batch_async: the host side of a solve (its round loop) on a worker thread of the handle
    struct AsyncJob { int B; const double *x0, *cl; const int32_t *cl_index; double *U, *lambda, *stats; void *stream; };
    std::thread worker;
    std::mutex mu;
    std::condition_variable cv;
    AsyncJob job{};
    bool job_posted = false, job_running = false, job_done = false, worker_quit = false;
    int job_rc = MPC_OK;
    std::string job_err;
    int ngroups = 0; // 0 = choose from the batch size
    int groups_last = 0; // sub-batch groups of the last solve
    long long round_limit = 0; // mpc_set_round_limit: cap on the rounds / persistent-kernel trips of a solve (0 = the guard alone)
    int hw_queues = 4; // streams of this process the HIP runtime runs side by side: 5 (or more) / 4 (or fewer), measured once per
                       // process and device (probe_stream_concurrency)
    double poll_timeout_s = 300.0; // wall-clock bound of a solve's host waits (mpc_set_poll_timeout / MPC_POLL_TIMEOUT_S): the
                                   // round loop gives up when no polled window has completed for this long, the blocking waits
                                   // behind it when they have lasted this long.  A valid solve never comes near it.
    bool timed_out = false;        // the last solve ended on that bound: work may still be queued on the device
    hipEvent_t syncev = nullptr;   // bounded_sync
    hipStream_t gstream[MPC_MAX_GROUPS] = {};
    hipEvent_t gevent[MPC_MAX_GROUPS + 1] = {};
    int check_every = 8;           // rounds per polled window of the round loop (MPC_CHECK_EVERY)
    bool spin = false;             // the round loop busy-waits instead of napping (MPC_SPIN)
    bool host_timing = false;      // the round loop prints its host-side times to stderr (MPC_HOST_TIMING)
    std::string host_trace;        // file the round loop appends one line per polled window to (MPC_HOST_TRACE; empty: none)
    // The caller's per-agent tables, one per kind (mpc_set_agent_params / _bounds / _constraints / _discs / _rates / _fields / _roads; device memory, read at
    // every call).  A kind with none bound runs the handle's values through the kernels that have always run.
    BoundTable tab[TAB_KINDS];
    const int32_t *pidx_plant = nullptr;   // parameters alone: [B] the plant's row per agent (mpc_closed_loop), null: the controller's
    const BoundTable &params() const { return tab[TAB_PARAMS]; }
    const int32_t *plant_rows() const { return pidx_plant ? pidx_plant : params().idx; }
    AgentIdx bound_rows() const { AgentIdx r; for (int k = 0; k < TAB_KINDS; k++) r.of[k] = tab[k].idx; return r; }
    // the bound tables into workspace `w` for agents whose rows are idx.of[kind][b] (a kind with no table bound: nulls, and
    // idx.of[kind] is not read) -- every kind, for every caller: what a kernel form does not read it is not handed
    void bind_tables(WorkspaceHost &w, const AgentIdx &idx) const
    {
        w.ptab = params().table; w.pidx = params().table ? idx.of[TAB_PARAMS] : nullptr;
        for (int k = TAB_BOX; k < TAB_KINDS; k++) w.tabs[k] = {tab[k].table, tab[k].table ? idx.of[k] : nullptr};
    }
    size_t table_width(int kind) const { return (size_t)k_tables[kind].width + (size_t)k_tables[kind].width_per_N * (size_t)cfg.N; }
    // The persistent kernel has its box form together with the parameter form alone, and its constraint form -- as the
    // K1 kernels have theirs -- together with both.  With a table bound but not the ones its kernels come with, they run
    // on these one-row tables of the handle's own values (bit for bit the shared path: tests/test_gpu_agent_params.py,
    // tests/test_gpu_agent_bounds.py) and an index of zeros; made at the first such bind, one allocation.
    OwnTables own;
    DevBuf stage;                          // the loops' statistics when the caller passes no buffer for them
    EventBufs ev;                          // mpc_solve_active / mpc_closed_loop_event
    TrafficBufs tr;                        // mpc_closed_loop_traffic and the obstacle loops
    ObstacleRuleBufs orule;                // mpc_closed_loop_obstacles_event
};

static int stage_m(const mpc_config *c)
{
    return c->constr_mode == MPC_CONSTR_STATE_SQ ? mpc_nx(c) : c->constr_mode == MPC_CONSTR_LANE ? 1 : c->constr_mode == MPC_CONSTR_DISCS ? MPC_NDISC : 0;
}

// the input box rule of mpc_create and mpc_set_agent_bounds: u_lb[i] <= u_ub[i] (a NaN fails it, infinities pass)
static bool box_ok(const double *lb, const double *ub)
{
    for (int i = 0; i < 2; i++)
        if (!(lb[i] <= ub[i])) return false;
    return true;
}

static int make_devcfg(const mpc_config &c, DevCfg &d)
{
    if (c.N < 1 || c.N > MPC_MAX_N) return fail(MPC_E_ARG, "horizon N out of range [1, 64]");
    if (c.S < 3) return fail(MPC_E_ARG, "centerline needs S >= 3 points");
    if (c.nfe < 1 || c.nfe > 16) return fail(MPC_E_ARG, "nfe out of range [1, 16]");
    if (c.lbfgs_memory < 1 || c.lbfgs_memory > 64) return fail(MPC_E_ARG, "lbfgs_memory out of range [1, 64]");
    if (c.model != MPC_MODEL_KINEMATIC && c.model != MPC_MODEL_PACEJKA) return fail(MPC_E_ARG, "unknown model");
    if (c.constr_mode < 0 || c.constr_mode > MPC_CONSTR_DISCS) return fail(MPC_E_ARG, "unknown constr_mode");
    if (c.max_no_progress < 1) return fail(MPC_E_ARG, "max_no_progress must be >= 1");
    if (c.max_iter < 1 || c.max_outer < 1 || c.max_total_inner < 1 || c.max_total_evals < 0)
        return fail(MPC_E_ARG, "max_iter, max_outer, max_total_inner must be >= 1 and max_total_evals >= 0");
    if (c.max_num_initial_retries < 0 || c.max_num_retries < 0 || c.max_total_num_retries < 0)
        return fail(MPC_E_ARG, "retry limits must be >= 0");
    if (!(c.Ts > 0.0) || !std::isfinite(c.Ts)) return fail(MPC_E_ARG, "Ts must be positive and finite");
    // alpaqa has a separate initial-penalty path for Sigma_0 == 0; it is not restated here
    if (!(c.Sigma0 > 0.0) || !(c.Sigma_max >= c.Sigma0) || !(c.M >= 0.0))
        return fail(MPC_E_ARG, "need 0 < Sigma0 <= Sigma_max and M >= 0");
    if (!(c.L_min > 0.0) || !(c.L_min <= c.L_max)) return fail(MPC_E_ARG, "need 0 < L_min <= L_max");
    if (!(c.alm_eps > 0.0) || !(c.alm_delta > 0.0) || !(c.eps0 > 0.0))
        return fail(MPC_E_ARG, "tolerances alm_eps, alm_delta, eps0 must be positive");
    if (!(c.tau_min > 0.0) || !(c.tau_min <= 1.0)) return fail(MPC_E_ARG, "tau_min must be in (0, 1]");
    if (!(c.Lgamma_factor > 0.0) || !(c.Lgamma_factor < 1.0)) return fail(MPC_E_ARG, "Lgamma_factor must be in (0, 1)");
    if (!box_ok(c.u_lb, c.u_ub)) return fail(MPC_E_ARG, "input box: u_lb must not exceed u_ub");
    std::memset(&d, 0, sizeof d);
    d.model = c.model; d.N = c.N; d.S = c.S; d.nfe = c.nfe; d.wrap_mode = c.wrap_mode;
    d.clip_inputs = c.clip_inputs; d.constr_mode = c.constr_mode; d.sm = stage_m(&c);
    d.nx = mpc_nx(&c); d.n = 2 * c.N; d.m = d.sm * c.N; d.M = c.lbfgs_memory;
    d.max_iter = c.max_iter; d.max_outer = c.max_outer; d.hess_heuristic = c.hess_heuristic;
    d.max_no_progress = c.max_no_progress;
    d.max_num_initial_retries = c.max_num_initial_retries; d.max_num_retries = c.max_num_retries;
    d.max_total_num_retries = c.max_total_num_retries; d.max_total_inner = c.max_total_inner;
    d.max_total_evals = c.max_total_evals;
    d.h = c.Ts / c.nfe; d.v_ref = c.v_ref;
    for (int i = 0; i < 6; i++) { d.w[i] = c.cost_w[i]; d.g_off[i] = c.g_off[i]; d.D_lb[i] = c.D_lb[i]; d.D_ub[i] = c.D_ub[i]; }
    d.lf = c.veh[1]; d.lr = c.veh[2]; d.mass = c.veh[7]; d.inv_mass = 1.0 / c.veh[7]; d.inv_iz = 1.0 / c.veh[8];
    d.max_steer = c.veh[9]; d.max_drive = c.veh[10];
    d.bf = c.veh[11]; d.cf = c.veh[12]; d.df = c.veh[13]; d.br = c.veh[14]; d.cr = c.veh[15]; d.dr = c.veh[16];
    d.cm1 = c.veh[17]; d.cm2 = c.veh[18]; d.cr0 = c.veh[19]; d.cr2 = c.veh[21];
    d.accel = c.accel; d.friction = c.friction;
    for (int i = 0; i < 2; i++) { d.u_lb[i] = c.u_lb[i]; d.u_ub[i] = c.u_ub[i]; }
    d.lane_hw = c.lane_halfwidth;
    // keep-out discs: g >= 0 for every agent and disc -- the bounds constraint_bounds serves K1b and the state machine with
    // (the configuration's g_off / D_lb / D_ub are STATE_SQ's and are not read in this mode)
    if (c.constr_mode == MPC_CONSTR_DISCS)
        for (int i = 0; i < MPC_NDISC; i++) { d.D_lb[i] = 0.0; d.D_ub[i] = INFINITY; }
    d.alm_eps = c.alm_eps; d.alm_delta = c.alm_delta; d.Sigma0 = c.Sigma0; d.eps0 = c.eps0; d.rho = c.rho;
    d.Delta = c.Delta; d.theta = c.theta; d.Mcap = c.M; d.Sigma_max = c.Sigma_max;
    d.Delta_lower = c.Delta_lower; d.Sigma0_lower = c.Sigma0_lower; d.eps0_increase = c.eps0_increase;
    d.rho_increase = c.rho_increase;
    d.lip_eps = c.lip_eps; d.lip_delta = c.lip_delta; d.Lgamma = c.Lgamma_factor; d.L_min = c.L_min;
    d.L_max = c.L_max; d.tau_min = c.tau_min; d.qub_tol = c.qub_tol;
    return MPC_OK;
}

// How many of this process's streams the HIP runtime runs side by side.  It maps streams to
// GPU_MAX_HW_QUEUES hardware queues (4 unless its environment said otherwise WHEN IT INITIALISED -- the
// variable as this process sees it now may have been set too late to count), and two streams that share a
// queue serialise: four sub-batch groups beside the caller's stream on four queues cost 259.8 ms per solve
// against 169.8 ms for three.  So the group count is decided on what is measured here, once
// per handle: a kernel that idles for a fixed time on the caller-side null stream and on the four group
// streams; side by side they take one such time, sharing a queue two.
__global__ void spin_kernel(long long ticks)
{
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}
static int probe_stream_concurrency_once(int device)
{
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz <= 0) khz = 100000;
    const double spin_us = 250.0;
    const long long ticks = (long long)(spin_us * 1e-6 * khz * 1e3);
    // five private non-blocking streams (not the null stream: a probe must neither wait for nor hold up the caller's
    // other streams, and must work while the caller is capturing a graph elsewhere); only they are synchronised
    hipStream_t st[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int result = 4;
    bool ok = true;
    for (int k = 0; k < 5 && ok; k++) ok = hipStreamCreateWithFlags(&st[k], hipStreamNonBlocking) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, st[0], 1LL);    // code object load, first-launch costs
        ok = hipStreamSynchronize(st[0]) == hipSuccess;
    }
    double best = 1e30;
    // three samples; when even the best of them looks like a shared queue AND like a busy device (more than three spins:
    // another handle's solve was running beside the probe), sample again a few times before settling for "four"
    for (int rep = 0; rep < 9 && ok; rep++) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < 5; k++) hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, st[k], ticks);
        for (int k = 0; k < 5 && ok; k++) ok = hipStreamSynchronize(st[k]) == hipSuccess;
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        best = std::min(best, us);
        if (rep >= 2 && !(best > 3.0 * spin_us)) break;
    }
    (void)hipGetLastError();
    for (int k = 0; k < 5; k++) if (st[k]) (void)hipStreamDestroy(st[k]);
    // five side by side: ~ one spin (+ launch overheads); a shared queue: two spins or more
    if (ok) result = best < 1.6 * spin_us ? 5 : 4;
    return result;
}
// measured once per (process, device): the answer is a property of the runtime's queue setup, not of the handle, and a
// handle created while another one is solving must not keep a pessimistic sample for its lifetime
static int probe_stream_concurrency(mpc_handle *h)
{
    static std::mutex mu;
    static int cached[64];
    std::lock_guard<std::mutex> lk(mu);
    const int d = h->device >= 0 && h->device < 64 ? h->device : 0;
    if (cached[d] == 0) cached[d] = probe_stream_concurrency_once(h->device);
    return cached[d];
}

// The library's environment switches (README.md has the table), read once per handle by mpc_create and nowhere else:
// they set handle fields and, from them, the DevCfg flags the kernels test.  None of them changes a result bit.
static void read_switches(mpc_handle *h)
{
    const auto num = [](const char *e, int &v) { if (e) v = atoi(e); };
    DevCfg &d = h->dc;
    d.no_spec = getenv("MPC_NO_SPEC") != nullptr;
    // which speculative gradients are not issued (DevCfg::spec_policy, spec_retry): 0 none, 1 the ones the line search or
    // the stop test is known to throw away, 2 also those of descent-lemma retries in the launches that carry chain blocks (launch_step_t)
    d.spec_policy = 2;
    num(getenv("MPC_SPEC_POLICY"), d.spec_policy);
    d.spec_policy = std::max(0, std::min(2, d.spec_policy));
    d.spec_retry = 0;
    num(getenv("MPC_SPEC_DEPTH"), h->spec_depth);
    h->spec_depth = std::max(1, std::min(30, h->spec_depth));
    d.no_memo = getenv("MPC_NO_MEMO") != nullptr;
    d.no_la = getenv("MPC_NO_LOOKAHEAD") != nullptr;
    d.all_rows = getenv("MPC_ALL_ROWS") != nullptr;
    // thread-per-agent chain blocks (MPC_NO_CHAIN: never; which launches carry them is decided per launch: chain_min).
    // Kinematic model only by default: measured on the Pacejka model, whose rounds wait for the rollout, 668 -> 699 ms per
    // solve with them; MPC_CHAIN_MIN set explicitly turns them on for either model.
    const char *chain_min = getenv("MPC_CHAIN_MIN");
    num(chain_min, h->chain_min);
    d.chain = getenv("MPC_NO_CHAIN") == nullptr && d.n <= 64 && (h->cfg.model == MPC_MODEL_KINEMATIC || chain_min != nullptr);
    h->step_regs = getenv("MPC_STEP_REGS") != nullptr;
    num(getenv("MPC_LDS_PAIRS"), h->lds_pairs);
    h->quad_rollout = getenv("MPC_NO_QUAD") == nullptr;
    num(getenv("MPC_PAC_QUAD_MAX"), h->pac_quad_max);
    num(getenv("MPC_WIDE_MAX"), h->wide_max);
    num(getenv("MPC_APB"), h->apb_env);
    h->fused_eval = getenv("MPC_UNFUSED_EVAL") == nullptr;
    num(getenv("MPC_FUSED_MAX"), h->fused_max);
    if (const char *e = getenv("MPC_SOLO_MAX")) h->solo_max = h->solo_all = atoi(e);
    num(getenv("MPC_SOLO_ALL"), h->solo_all);
    if (getenv("MPC_NEAREST_SCAN")) h->nearest_mode = 0;
    const char *p = getenv("MPC_PROFILE");
    h->profile = p && p[0] == '1';
    if (const char *e = getenv("MPC_POLL_TIMEOUT_S")) { const double t = atof(e); if (t > 0.0) h->poll_timeout_s = t; }
    num(getenv("MPC_GROUPS"), h->ngroups);
    int check = 0;
    num(getenv("MPC_CHECK_EVERY"), check);
    if (check > 0) h->check_every = check;
    h->spin = getenv("MPC_SPIN") != nullptr;
    h->host_timing = getenv("MPC_HOST_TIMING") != nullptr;
    if (const char *e = getenv("MPC_HOST_TRACE")) h->host_trace = e;
    // (MPC_HW_QUEUES overrides the measurement: experiments only)
    const char *hwq = getenv("MPC_HW_QUEUES");
    h->hw_queues = hwq ? atoi(hwq) : probe_stream_concurrency(h);
}

// the workspace for up to B agents (agent-major rows; caller buffers are used in place)
static int reserve(mpc_handle *h, int B)
{
    const int Bp = (int)pad64((size_t)B);
    if (Bp <= h->Bp_alloc) { h->ws.Bp = h->Bp_alloc; h->ws.B = B; return MPC_OK; }
    WorkspaceHost &w = h->ws;
    h->Bp_alloc = 0;
    const int rc = carve(h->arena, h->device, true, "workspace hipMalloc failed: ",
                         [&](Carver &a) { workspace_layout(a, w, h->dc, (size_t)Bp); });
    if (rc) return rc;
    h->Bp_alloc = Bp;
    w.Bp = Bp; w.B = B; w.St = (int)ws_slots((size_t)Bp); w.Ls = Bp;
    w.ws_xe = w.xe; w.ws_ge = w.ge; w.ws_yhe = w.yhe; w.ws_Sig = w.Sig;
    return MPC_OK;
}

static int reserve_stage(mpc_handle *h, size_t bytes) { return h->stage.grow(h->device, bytes, false, "staging hipMalloc failed"); }

// One of the handle's *Bufs for up to B agents: its arena grown to layout(Carver &, bufs, dims..., capacity), zero-filled,
// and its pointers placed
template <class Bufs, class Layout, class... Dims>
static int reserve_bufs(mpc_handle *h, Bufs &b, int B, const char *msg, Layout layout, const Dims &...dims)
{
    if (B <= b.cap) return MPC_OK;
    const size_t Bp = pad64((size_t)B);
    b.cap = 0;
    const int rc = carve(b.arena, h->device, true, msg, [&](Carver &a) { layout(a, b, dims..., Bp); });
    if (rc == MPC_OK) b.cap = (int)Bp;
    return rc;
}
// staging of the masked solve (EventBufs), buffers of the traffic loop (TrafficBufs) and of the obstacle rule (ObstacleRuleBufs)
static int reserve_event(mpc_handle *h, int B) { return reserve_bufs(h, h->ev, B, "masked-solve staging hipMalloc failed", event_layout, h->dc); }
static int reserve_traffic(mpc_handle *h, int B) { return reserve_bufs(h, h->tr, B, "traffic-loop hipMalloc failed", traffic_layout, h->dc); }
static int reserve_obstacle_rule(mpc_handle *h, int B) { return reserve_bufs(h, h->orule, B, "obstacle-rule hipMalloc failed", obstacle_rule_layout); }
// the nominal states for a batch of B agents; *fresh = they were (re)allocated: no agent's nominal state is known
static int reserve_xhat(mpc_handle *h, int B, bool *fresh)
{
    EventBufs &e = h->ev;
    *fresh = false;
    if (e.xhat && e.xhat_B == B) return MPC_OK;
    HIPCHK(e.xhat_mem.release());           // (a batch of another size, a smaller one too: none of the states is this batch's)
    e.xhat = nullptr; e.xhat_B = 0;
    const int rc = e.xhat_mem.grow(h->device, sizeof(double) * (size_t)B * h->dc.nx, true, "nominal-state hipMalloc failed", fresh);
    if (rc) return rc;
    e.xhat = (double *)e.xhat_mem.p; e.xhat_B = B;
    return MPC_OK;
}
// the handle's own one-row parameter, box, rate and field tables and an index of B zeros (see mpc_handle::own): the rows
// are laid out and filled on the host and copied with the zeros behind them
static int reserve_own_tables(mpc_handle *h, int B, const char *who)
{
    OwnTables &o = h->own;
    if (B <= o.cap) return MPC_OK;
    const size_t cap = pad64((size_t)B);
    o.cap = 0;
    const int rc = carve(o.arena, h->device, false, std::string(who) + ": hipMalloc failed",
                         [&](Carver &a) { own_tables_layout(a, o, h->cfg.N, cap); });
    if (rc) return rc;
    std::vector<double> host((o.arena.bytes + 7) / 8, 0.0);
    OwnTables rows;
    Carver on_host((char *)host.data());
    own_tables_layout(on_host, rows, h->cfg.N, cap);
    (void)mpc_default_params(&h->cfg, rows.ptab);
    (void)mpc_default_bounds(&h->cfg, rows.btab);
    (void)mpc_default_rates(&h->cfg, rows.rtab);
    (void)mpc_default_fields(&h->cfg, rows.ftab);
    HIPCHK(hipMemcpy(o.arena.p, host.data(), o.arena.bytes, hipMemcpyHostToDevice));
    o.cap = (int)cap;
    return MPC_OK;
}

// A handle with a table bound serves the batch size the table's indices were bound for, and no other, in the calls
// that read that kind of table (`kinds`: a mask of READS_*).  Parameters, box, constraints, discs, rates, fields, roads: the first mismatch wins.
// The discs have no shared values to fall back on: a call that evaluates constraints (`needs_discs`) on a handle of
// MPC_CONSTR_DISCS with no disc table bound is refused.
static int check_tables(const mpc_handle *h, int B, const char *who, unsigned kinds, bool needs_discs = false)
{
    if (needs_discs && h->cfg.constr_mode == MPC_CONSTR_DISCS && !h->tab[TAB_DISCS].table)
        return fail(MPC_E_ARG, std::string(who) + ": the handle's constraints are keep-out discs (MPC_CONSTR_DISCS) and no disc table is bound (" +
                               k_tables[TAB_DISCS].setter + ")");
    for (int k = 0; k < TAB_KINDS; k++) {
        const BoundTable &t = h->tab[k];
        if ((kinds >> k & 1u) && t.table && B != t.B)
            return fail(MPC_E_ARG, std::string(who) + ": the bound " + k_tables[k].noun + " table is for a batch of " + std::to_string(t.B) +
                                   " agents, this call has " + std::to_string(B) + " (" + k_tables[k].setter + ")");
    }
    return MPC_OK;
}
// a table can be bound for B agents beside the ones that are: bound together they are for the same batch
// (self: the kind being bound, whose earlier binding does not count)
static int check_tables_agree(const mpc_handle *h, int B, const char *who, int self)
{
    for (int k = 0; k < TAB_KINDS; k++) {
        const BoundTable &t = h->tab[k];
        if (k != self && t.table && t.B != B)
            return fail(MPC_E_ARG, std::string(who) + ": the bound " + k_tables[k].noun + " table is for a batch of " + std::to_string(t.B) + " agents");
    }
    return MPC_OK;
}
static inline dim3 grid_for(int B, int block) { return dim3((unsigned)((B + block - 1) / block)); }

// Every entry point that touches the handle's tables, workspace or streams goes through here.  While an
// asynchronous solve is posted, running or waiting to be collected (mpc_solve_batch_async .. mpc_solve_wait)
// the worker thread owns the handle: anything else is refused BEFORE it touches the handle (a second
// mpc_centerline_blocks would free or overwrite the search tables under the running solve's kernels).
static int refuse_if_busy(mpc_handle *h, const char *who)
{
    if (!h) return fail(MPC_E_ARG, std::string(who) + ": null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->job_posted || h->job_running || h->job_done)
        return fail(MPC_E_ARG, std::string(who) + ": a solve of this handle is in flight (mpc_solve_wait first)");
    return MPC_OK;
}
static int check_common(mpc_handle *h, int B, const char *who, bool from_worker = false)
{
    if (!h) return fail(MPC_E_ARG, std::string(who) + ": null handle");
    if (B < 0) return fail(MPC_E_ARG, std::string(who) + ": negative batch");
    if (!from_worker) { const int rb = refuse_if_busy(h, who); if (rb) return rb; }
    HIPCHK(hipSetDevice(h->device));
    return MPC_OK;
}

// the search tables to use with centerline table `cl` (all null: none prepared for it, or switched off)
static NearTab near_for(const mpc_handle *h, const double *cl)
{
    NearTab nt = {nullptr, nullptr, nullptr};
    if (h->nearest_mode == 2 && h->cl_grid_for && h->cl_grid_for == cl) { nt.gmeta = h->grid.gmeta; nt.gcells = h->grid.gcells; nt.gxy = h->grid.gxy; }
    return nt;
}

static hipEvent_t get_event(mpc_handle *h, size_t i)
{
    while (h->ev_pool.size() <= i) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        h->ev_pool.push_back(e);
    }
    return h->ev_pool[i];
}

// hipStreamSynchronize with the handle's wall-clock bound: an event behind everything queued on `s`, polled in naps.
// Returns MPC_OK, or MPC_E_HIP with h->timed_out set when the bound expired (work is then still queued).
static int bounded_sync(mpc_handle *h, hipStream_t s, const char *what)
{
    if (!h->syncev) HIPCHK(hipEventCreateWithFlags(&h->syncev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(h->syncev, s));
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipEventQuery(h->syncev);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) return fail(MPC_E_HIP, std::string(what) + ": " + hipGetErrorString(q));
        const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (waited > h->poll_timeout_s) {
            h->timed_out = true;
            return fail(MPC_E_HIP, std::string(what) + ": wall-clock bound of " + std::to_string(h->poll_timeout_s) +
                                   " s expired while waiting for the device (mpc_set_poll_timeout); work is still queued");
        }
        if (waited < 100e-6) __builtin_ia32_pause();
        else std::this_thread::sleep_for(std::chrono::microseconds(waited < 5e-3 ? 20 : 200));
    }
    (void)hipGetLastError();   // (the queries that said "not ready" left that as the thread's last error)
    return MPC_OK;
}
