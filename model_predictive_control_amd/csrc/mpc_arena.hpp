// mpc_arena.hpp -- host side of libmpc_hip.so, part 0: error reporting, the owner of one allocation (DevBuf) and the
// layout of everything the handle carves out of one: a function per arena, walked twice by a Carver -- without a base it
// measures, with the allocation it places the pointers -- so that no size is written beside the carving it has to
// cover.  Host code with no HIP call outside DevBuf; included by mpc_handle.hpp (and by the layout test's program).
#pragma once
#include "../../include/mpc_hip.h"
#include "mpc_event.hpp"

#include <cstddef>
#include <string>

using namespace mpc;

#define MPC_MAX_GROUPS 8

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(MPC_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));        \
    } while (0)

// One device allocation (pinned host memory with `pinned`) and its size; freed with its owner.
struct DevBuf {
    char *p = nullptr;
    size_t bytes = 0;
    const bool pinned;
    explicit DevBuf(bool pinned_ = false) : pinned(pinned_) {}
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { (void)release(); }
    hipError_t release()
    {
        const hipError_t e = !p ? hipSuccess : pinned ? hipHostFree(p) : hipFree(p);
        p = nullptr; bytes = 0;
        return e;
    }
    hipError_t alloc(size_t n)   // n bytes in place of what is held
    {
        hipError_t e = release();
        if (e == hipSuccess) e = pinned ? hipHostMalloc((void **)&p, n, hipHostMallocDefault) : hipMalloc((void **)&p, n);
        if (e == hipSuccess) bytes = n; else p = nullptr;
        return e;
    }
    // At least n bytes: what is held when it is enough, else a new allocation on `device` (zero-filled with `zero`) in
    // its place -- the old contents are gone -- and *grew = true.  No memory: MPC_E_ALLOC with `msg` (one that ends in
    // ": " gets HIP's reason behind it).
    int grow(int device, size_t n, bool zero, const std::string &msg, bool *grew = nullptr)
    {
        if (grew) *grew = false;
        if (n <= bytes) return MPC_OK;
        HIPCHK(hipSetDevice(device));
        HIPCHK(release());
        const hipError_t e = alloc(n);
        if (e != hipSuccess) return fail(MPC_E_ALLOC, msg.back() == ' ' ? msg + hipGetErrorString(e) : msg);
        if (zero) HIPCHK(hipMemset(p, 0, n));
        if (grew) *grew = true;
        return MPC_OK;
    }
};

// Walks a layout: take(dst, count) is the next block, `count` elements aligned to their type.  Without a base nothing
// is written and `off` ends as the size the layout needs; with one, dst points into it.
struct Carver {
    char *const base;
    size_t off = 0;
    explicit Carver(char *base_ = nullptr) : base(base_) {}
    template <class T> void take(T *&dst, size_t count)
    {
        off = (off + alignof(T) - 1) / alignof(T) * alignof(T);
        if (base) dst = reinterpret_cast<T *>(base + off);
        off += count * sizeof(T);
    }
};
// grows `buf` to what `layout(Carver &)` measures and places the layout's pointers on it
template <class Layout>
static int carve(DevBuf &buf, int device, bool zero, const std::string &msg, Layout layout)
{
    Carver measure;
    layout(measure);
    const int rc = buf.grow(device, measure.off, zero, msg);
    if (rc) return rc;
    Carver place(buf.p);
    layout(place);
    return MPC_OK;
}
static inline size_t pad64(size_t B) { return (B + 63) & ~(size_t)63; }   // capacities are whole waves of agents

// ------------------------------------------------------------------------------------------------ the workspace
// slots of the K1 scratch: a round holds at most two requests per agent (cost + speculative gradient), and every
// group's slots start on a multiple of 64
static inline size_t ws_slots(size_t Bp) { return 2 * Bp + 64 * (MPC_MAX_GROUPS + 1); }
// what SolveRun::begin clears in one piece: Workspace::counts (8 ints per group), totals and solo_ctr
struct DevCounters {
    int counts[8 * MPC_MAX_GROUPS];
    unsigned long long totals[16];
    int solo_ctr[2 * MPC_MAX_GROUPS];          // [group][claim counter, list length]
};
static_assert(offsetof(DevCounters, counts) == 0, "SolveRun::begin clears sizeof(DevCounters) from Workspace::counts");
// the arrays of Workspace that are the handle's own, for a capacity of Bp agents (agent-major rows, then the
// slot-indexed K1 scratch, then the lists and counters)
static void workspace_layout(Carver &a, Workspace &w, const DevCfg &c, size_t Bp)
{
    const size_t n = c.n, m = c.m ? c.m : 1, M = c.M, nx = c.nx, N = c.N, JS = nx * (nx + 1) + 2, St = ws_slots(Bp);
    for (double **v : {&w.xk, &w.gk, &w.q, &w.xn, &w.xe, &w.ge, &w.xe2, &w.ge2}) a.take(*v, n * Bp);
    a.take(w.S, M * n * Bp); a.take(w.Y, M * n * Bp);
    for (double **v : {&w.Sig, &w.Sig_old, &w.e1, &w.e2, &w.yhx, &w.yhxn, &w.yhe}) a.take(*v, m * Bp);
    a.take(w.rec, REC * Bp);
    a.take(w.trajx, (N + 1) * nx * St); a.take(w.useq, 2 * N * St); a.take(w.stage_L, N * St); a.take(w.jac, N * JS * St);
    a.take(w.lists, 4 * Bp);
    a.take(w.agent_of, St);
    DevCounters *ctr = nullptr;
    a.take(ctr, 1);
    if (ctr) { w.counts = ctr->counts; w.totals = ctr->totals; w.solo_ctr = ctr->solo_ctr; }
}

// ---------------------------------------------------------------------------------- the arenas of the entry points
// The per-agent tables a caller can bind beside the handle's shared values: parameters (mpc_set_agent_params), input
// boxes (mpc_set_agent_bounds), constraint data (mpc_set_agent_constraints), keep-out discs (mpc_set_agent_discs) and move
// penalties (mpc_set_agent_rates), risk fields (mpc_set_agent_fields) and road data (mpc_set_agent_roads).  The kinds are walked in this order wherever they are checked; an entry point names the kinds it reads as a mask of READS_*
// (check_tables in mpc_handle.hpp).
enum TableKind { TAB_PARAMS, TAB_BOX, TAB_CONSTR, TAB_DISCS, TAB_RATES, TAB_FIELDS, TAB_ROADS, TAB_KINDS };

// mpc_solve_active / mpc_closed_loop_event: the compaction's list and counters, the staging rows the active agents
// are solved on (one allocation, grown like the workspace), and the nominal states of the event-triggered loop
// (their own allocation: they are STATE between calls and must outlive a regrown staging arena)
struct EventBufs {
    DevBuf arena;
    int cap = 0;                                   // agents the arena holds
    int *list = nullptr, *blk = nullptr, *count = nullptr, *fire = nullptr, *cis = nullptr;
    int *rows[TAB_KINDS] = {};                     // the active agents' rows of the bound tables, by kind
    double *xs = nullptr, *Us = nullptr, *lams = nullptr, *stats_s = nullptr, *stats_own = nullptr;
    DevBuf xhat_mem;
    double *xhat = nullptr;                        // [xhat_B][nx], all of xhat_mem
    int xhat_B = 0;
};
static void event_layout(Carver &a, EventBufs &e, const DevCfg &c, size_t Bp)
{
    a.take(e.xs, c.nx * Bp); a.take(e.Us, c.n * Bp); a.take(e.lams, (c.m ? c.m : 1) * Bp);
    a.take(e.stats_s, 8 * Bp); a.take(e.stats_own, 8 * Bp);
    a.take(e.list, Bp); a.take(e.fire, Bp); a.take(e.cis, Bp);
    for (int *&rows : e.rows) a.take(rows, Bp);
    a.take(e.blk, (Bp + EV_BLK - 1) / EV_BLK);
    a.take(e.count, 64);
}

// mpc_closed_loop_traffic: everybody's plans X [cap][N][nx] of the step and the opponents chosen from them
// [cap][MPC_NDISC] (one allocation, grown like the workspace)
struct TrafficBufs {
    DevBuf arena;
    int cap = 0;
    double *X = nullptr;
    int32_t *opp = nullptr;
};
static void traffic_layout(Carver &a, TrafficBufs &t, const DevCfg &c, size_t Bp)
{
    a.take(t.X, (size_t)c.N * c.nx * Bp);
    a.take(t.opp, MPC_NDISC * Bp);
}

// mpc_closed_loop_obstacles_event: the selection over the stages every plan still holds, sel_chk [cap][MPC_NDISC] and
// clear_chk [cap][MPC_NDISC] (what mpc_obstacle_trigger's caller passes)
struct ObstacleRuleBufs {
    DevBuf arena;
    int cap = 0;
    double *clear_chk = nullptr;
    int32_t *sel_chk = nullptr;
};
static void obstacle_rule_layout(Carver &a, ObstacleRuleBufs &o, size_t Bp)
{
    a.take(o.clear_chk, MPC_NDISC * Bp);
    a.take(o.sel_chk, MPC_NDISC * Bp);
}

// The handle's own one-row tables (see mpc_handle::own) and an index of `cap` zeros.  The layout is walked over host
// memory too: the rows are filled there and copied in one piece.
struct OwnTables {
    DevBuf arena;
    int cap = 0;
    double *ptab = nullptr;                // [MPC_NPARAM] and a pad
    double *btab = nullptr;                // [MPC_NBOUND]
    double *rtab = nullptr;                // [MPC_NRATE] zeros: no move penalty (the field forms stand behind the rate forms alone)
    double *ftab = nullptr;                // [MPC_FIELD_ROW(N)] zeros: no source (the road forms of a handle without discs stand behind the field forms alone)
    int32_t *pidx = nullptr;               // [cap] zeros
};
static void own_tables_layout(Carver &a, OwnTables &o, int N, size_t cap)
{
    a.take(o.ptab, MPC_NPARAM + 1); a.take(o.btab, MPC_NBOUND); a.take(o.rtab, MPC_NRATE); a.take(o.ftab, MPC_FIELD_ROW(N));
    a.take(o.pidx, cap);
}

// the grid of index ranges of the centerline table last handed to mpc_centerline_blocks, for C rows of S points
struct GridBufs {
    DevBuf arena;
    int cap = 0;                                     // rows the grid holds
    double *gmeta = nullptr, *gxy = nullptr;         // grid placement [C][GRID_META], interleaved points [C][S][2]
    unsigned *gcells = nullptr;                      // [C][GRID_CELLS]
};
static void grid_layout(Carver &a, GridBufs &g, size_t S, size_t C)
{
    a.take(g.gmeta, GRID_META * C); a.take(g.gxy, 2 * S * C); a.take(g.gcells, (size_t)GRID_CELLS * C);
}

// ------------------------------------------------------------------------------------------- the pinned block
// What the device copies back for the host to read behind an event or a bounded wait -- copies into pageable memory
// would block the host until the stream has drained, whatever the wall-clock bound says.
struct PinnedCounts {
    int poll[2][MPC_MAX_GROUPS][2];            // the round loop: [polled window][group] the two request counts of its last round
    unsigned long long totals[16];             // Workspace::totals of a solve
    int solo_ctr[2 * MPC_MAX_GROUPS];          // Workspace::solo_ctr of a solve
    char pad[64];
    int n_active;                              // the masked solve's count
    char tail[124];
};
static_assert(sizeof(PinnedCounts) == 512 && offsetof(PinnedCounts, poll) == 0 && offsetof(PinnedCounts, totals) == 128 &&
              offsetof(PinnedCounts, solo_ctr) == 256 && offsetof(PinnedCounts, n_active) == 384, "pinned block layout");
static_assert(sizeof(PinnedCounts::totals) == sizeof(DevCounters::totals) && sizeof(PinnedCounts::solo_ctr) == sizeof(DevCounters::solo_ctr),
              "the totals and the persistent kernel's counters are copied whole");
