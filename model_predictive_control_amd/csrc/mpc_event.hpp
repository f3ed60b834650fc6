// mpc_event.hpp -- kernels of the masked solve and the event-triggered closed loop (mpc_solve_active,
// mpc_trigger_eval, mpc_closed_loop_event): the stable compaction of an active mask into an agent list, the gather /
// scatter between the caller's batch and the handle's staging rows, the trigger and the per-step kernel that advances
// plant and nominal state.  The solver kernels are not touched: a masked solve IS the existing solve, run on the
// gathered rows (agents are independent, so a sliced batch gives the sliced result bit for bit).
#pragma once
#include "mpc_aux.hpp"

namespace mpc {

constexpr int EV_BLK = 256;   // threads per workgroup of the compaction kernels (four waves)

MPC_DEV int ev_wave_sum(int v)
{
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Compaction, pass 1: blk[g] = active agents among the EV_BLK agents of workgroup g (wave ballot + population count)
__global__ void __launch_bounds__(EV_BLK) active_count_kernel(int B, const int *__restrict__ active, int *__restrict__ blk)
{
    __shared__ int s_w[EV_BLK / 64];
    const int a = blockIdx.x * EV_BLK + threadIdx.x;
    const bool on = a < B && active[a] != 0;
    const unsigned long long m = __ballot(on);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// Compaction, pass 2: the index-ascending list.  Workgroup g starts at the sum of blk[0 .. g) (every workgroup sums
// that prefix itself: 256 counts at 65 536 agents), a wave at the counts of the waves before it, a lane at the set
// bits below it in its wave's ballot.  No atomics: the same mask gives the same list.  The last workgroup writes the
// total.
__global__ void __launch_bounds__(EV_BLK) active_list_kernel(int B, const int *__restrict__ active, const int *__restrict__ blk,
                                                             int *__restrict__ list, int *__restrict__ count)
{
    __shared__ int s_pre[EV_BLK / 64], s_w[EV_BLK / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int part = 0;
    for (int i = threadIdx.x; i < (int)blockIdx.x; i += EV_BLK) part += blk[i];
    part = ev_wave_sum(part);
    const int a = blockIdx.x * EV_BLK + threadIdx.x;
    const bool on = a < B && active[a] != 0;
    const unsigned long long m = __ballot(on);
    if (lane == 0) { s_pre[wv] = part; s_w[wv] = __popcll(m); }
    __syncthreads();
    int off = s_pre[0] + s_pre[1] + s_pre[2] + s_pre[3];
    for (int k = 0; k < wv; k++) off += s_w[k];
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    if (on) list[off + rank] = a;      // off + rank < number of active agents <= B
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == EV_BLK - 1) *count = off + s_w[EV_BLK / 64 - 1];
}

// the rows the masked solve moves between the caller's batch ([B] agents) and the staging rows ([count] agents)
struct ActiveRows {
    const int *list, *count;
    int nx, n, m;
    double *x0, *U, *lam, *stats;      // caller's (x0 is only read; lam null when m == 0; stats may be null)
    const int *cl_index, *pidx;        // caller's (either may be null)
    double *xs, *Us, *lams, *stats_s;  // staging
    int *cis, *pis;
};

// one wave per listed agent: x0, U, lambda, centerline row and parameter row into staging row i
__global__ void __launch_bounds__(EV_BLK) active_gather_kernel(const ActiveRows r)
{
    const int lane = threadIdx.x & 63, i = blockIdx.x * (EV_BLK / 64) + (threadIdx.x >> 6);
    if (i >= *r.count) return;
    const int a = r.list[i];
    for (int j = lane; j < r.nx; j += 64) r.xs[(size_t)i * r.nx + j] = r.x0[(size_t)a * r.nx + j];
    for (int j = lane; j < r.n; j += 64) r.Us[(size_t)i * r.n + j] = r.U[(size_t)a * r.n + j];
    for (int j = lane; j < r.m; j += 64) r.lams[(size_t)i * r.m + j] = r.lam[(size_t)a * r.m + j];
    if (lane == 0) {
        if (r.cl_index) r.cis[i] = r.cl_index[a];
        if (r.pidx) r.pis[i] = r.pidx[a];
    }
}

// the bounds-table (or constraint-table) row index of every listed agent into its staging row (one thread per listed
// agent; a launch of its own, made only while that table is bound: the gather above is what it was)
__global__ void __launch_bounds__(EV_BLK) active_index_kernel(const int *__restrict__ list, const int *__restrict__ count,
                                                              const int *__restrict__ src, int *__restrict__ dst)
{
    const int i = blockIdx.x * EV_BLK + threadIdx.x;
    if (i < *count) dst[i] = src[list[i]];
}

// ... and U, lambda and the statistics back; rows of agents that are not listed are not written
__global__ void __launch_bounds__(EV_BLK) active_scatter_kernel(const ActiveRows r)
{
    const int lane = threadIdx.x & 63, i = blockIdx.x * (EV_BLK / 64) + (threadIdx.x >> 6);
    if (i >= *r.count) return;
    const int a = r.list[i];
    for (int j = lane; j < r.n; j += 64) r.U[(size_t)a * r.n + j] = r.Us[(size_t)i * r.n + j];
    for (int j = lane; j < r.m; j += 64) r.lam[(size_t)a * r.m + j] = r.lams[(size_t)i * r.m + j];
    if (r.stats && lane < 8) r.stats[(size_t)a * 8 + lane] = r.stats_s[(size_t)i * 8 + lane];
}

// The trigger.  e = x - xhat, the heading component (index 2 in both models) reduced to (-pi, pi] by
// e -= 2 pi rint(e / 2 pi) (the models may wrap phi); dev2 = sum_i w_i e_i^2 in index order, every operation rounded
// on its own (contraction off: a host loop in IEEE doubles gets the same bits); fire = held < 0 || held >= max_hold ||
// dev2 >= thr2, written as !(dev2 < thr2) so that a non-finite dev2 fires.
struct TrigW { double w[6]; };
template <int NX> MPC_DEV double trigger_dev2(const double *__restrict__ x, const double *__restrict__ xhat, const TrigW &w)
{
#pragma clang fp contract(off)
    const double two_pi = 6.283185307179586476925286766559;
    double d2 = 0.0;
#pragma unroll
    for (int i = 0; i < NX; i++) {
        double e = x[i] - xhat[i];
        if (i == 2) e = e - two_pi * rint(e / two_pi);
        d2 = d2 + w.w[i] * (e * e);
    }
    return d2;
}
// a + b rounded once, never contracted with the operation that made a (the disturbance is added to the plant's state
// as a host loop adds it to mpc_rollout's result)
MPC_DEV double add_rounded(double a, double b)
{
#pragma clang fp contract(off)
    return a + b;
}
MPC_DEV bool trigger_fire(int held, int max_hold, double dev2, double thr2) { return held < 0 || held >= max_hold || !(dev2 < thr2); }

// the in-place shift of a plan Ua [N][2] by the hd > 0 stages that have been applied, the last stage repeated into the tail
MPC_DEV void plan_shift(double *Ua, int N, int hd)
{
    const int k = min(hd, N - 1);
    for (int j = 0; j < N; j++) {           // ascending: a stage is read before it is overwritten
        const int src = min(j + k, N - 1);
        Ua[2 * j] = Ua[2 * src]; Ua[2 * j + 1] = Ua[2 * src + 1];
    }
}

// mpc_trigger_eval, and step 1 - 2 of mpc_closed_loop_event (U != null: a firing agent's plan is shifted in place by
// the `held` stages it has applied, the last stage repeated into the tail -- `held` applications of plant_step_kernel's
// one-stage shift; force != 0: every agent fires, the nominal states are not known)
template <int NX>
__global__ void __launch_bounds__(64) trigger_kernel(int B, int N, const double *__restrict__ x, const double *__restrict__ xhat,
                                                     const int *__restrict__ held, const TrigW w, double thr2, int max_hold,
                                                     int force, double *__restrict__ dev2, int *__restrict__ fire,
                                                     double *__restrict__ U)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= B) return;
    const double d2 = trigger_dev2<NX>(x + (size_t)a * NX, xhat + (size_t)a * NX, w);
    const int hd = held[a];
    const bool f = force != 0 || trigger_fire(hd, max_hold, d2, thr2);
    if (dev2) dev2[a] = d2;
    fire[a] = f ? 1 : 0;
    if (U && f && hd > 0) plan_shift(U + (size_t)a * 2 * N, N, hd);
}

// step 4 of mpc_closed_loop_obstacles_event: the trigger's shift as a launch of its own, behind the obstacle rule -- the
// plans of the agents that fire for any reason are shifted by the stages they have applied (one thread per agent)
__global__ void __launch_bounds__(64) plan_shift_kernel(int B, int N, const int *__restrict__ held, const int *__restrict__ fire,
                                                        double *__restrict__ U)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= B) return;
    const int hd = held[a];
    if (fire[a] != 0 && hd > 0) plan_shift(U + (size_t)a * 2 * N, N, hd);
}

// plant's and controller's parameters of agent a: rows plant_index[a] and index[a] of the bound table
MPC_DEV void event_cfgs(DevCfg &cp, DevCfg &cc, const double *__restrict__ tab, const int *__restrict__ plant_index,
                        const int *__restrict__ index, int a)
{
    agent_cfg(cp, tab, plant_index, a);
    agent_cfg(cc, tab, index, a);
}

// Steps 3 - 5 of mpc_closed_loop_event for one agent per thread: an agent that fired has just been solved (held = 0,
// xhat = x); every agent applies stage `held` of its plan -- the plant x <- f_d(x, u) on the plant's row (+ the caller's
// disturbance), the nominal state xhat <- f_d(xhat, u) on the controller's row, both in this thread, so no predicted
// trajectory is stored or re-rolled -- and moves on one stage.  PA: pt = (table, plant_index, index).
template <int MODEL, bool PA = false, class... PT>
__global__ void __launch_bounds__(64) event_step_kernel(const DevCfg c_, int B, int t, int T, double *__restrict__ x,
                                  double *__restrict__ xhat, const double *__restrict__ U, int *__restrict__ held,
                                  const int *__restrict__ fire, const double *__restrict__ disturbance,
                                  double *__restrict__ traj_x, double *__restrict__ traj_u, uint8_t *__restrict__ solved,
                                  int *__restrict__ solve_count, const double *__restrict__ stats,
                                  int *__restrict__ fail_count, PT... pt)
{
    constexpr int NX = ModelDim<MODEL>::NX;
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= B) return;
    DevCfg cp_, cc_;
    if constexpr (PA) { cp_ = c_; cc_ = c_; event_cfgs(cp_, cc_, pt..., a); }
    const DevCfg &cp = PA ? cp_ : c_, &cc = PA ? cc_ : c_;
    const bool f = fire[a] != 0;
    int hd = f ? 0 : held[a];
    hd = max(0, min(hd, c_.N - 1));            // (a held agent has 0 <= held < max_hold <= N: the clamp guards the read)
    double xv[NX], xh[NX];
    for (int i = 0; i < NX; i++) xv[i] = x[(size_t)a * NX + i];
    for (int i = 0; i < NX; i++) xh[i] = f ? xv[i] : xhat[(size_t)a * NX + i];
    const double d = U[(size_t)a * c_.n + 2 * hd], dl = U[(size_t)a * c_.n + 2 * hd + 1];
    {
        StageInput<MODEL> s;
        prep_input(cp, d, dl, s);
        stage_forward<MODEL>(cp, s, xv);
    }
    if (disturbance)
        for (int i = 0; i < NX; i++) xv[i] = add_rounded(xv[i], disturbance[((size_t)a * T + t) * NX + i]);
    {
        StageInput<MODEL> s;
        prep_input(cc, d, dl, s);
        stage_forward<MODEL>(cc, s, xh);
    }
    for (int i = 0; i < NX; i++) {
        x[(size_t)a * NX + i] = xv[i];
        xhat[(size_t)a * NX + i] = xh[i];
        if (traj_x) traj_x[((size_t)a * T + t) * NX + i] = xv[i];
    }
    if (traj_u) { traj_u[((size_t)a * T + t) * 2] = d; traj_u[((size_t)a * T + t) * 2 + 1] = dl; }
    held[a] = hd + 1;
    if (solved) solved[(size_t)a * T + t] = f ? 1 : 0;
    if (f) {
        if (solve_count) solve_count[a] += 1;
        if (fail_count) fail_count[a] += stats[(size_t)a * 8] != (double)ST_CONVERGED;
    }
}

// mpc_set_agent_rates in the closed loops: the input about to be applied goes into columns 2 and 3 of the agent's row of the
// bound rate table -- u_{-1} of its next solve.  That is stage hd of the plan: hd = 0 in mpc_closed_loop(_traffic) (held
// and fire null); in the event loops the stage event_step_kernel is about to apply (0 for an agent that fired, held[a]
// otherwise, clamped as there).  Launched between the solve and the kernel that advances the plant (and may shift the
// plan).  Every word written is a copy of a word of U.  Rows are the agents' own: the loops require P == B.
__global__ void __launch_bounds__(64) rate_prev_kernel(int B, int N, const double *__restrict__ U, const int *__restrict__ held,
                                                       const int *__restrict__ fire, double *__restrict__ rtab,
                                                       const int *__restrict__ ridx)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= B) return;
    int hd = held && !(fire && fire[a] != 0) ? held[a] : 0;
    hd = max(0, min(hd, N - 1));
    double *r = rtab + (size_t)ridx[a] * NRATE;
    r[2] = U[(size_t)a * 2 * N + 2 * hd]; r[3] = U[(size_t)a * 2 * N + 2 * hd + 1];
}

// mpc_discs_from_plans: table[b][k][j] = (X[o][k][0], X[o][k][1], radius[o]) for o = opp[b][j], zeros where there is no such
// agent (o < 0 or o >= B).  One thread per (agent, stage, disc); every word written is a copy of an input word or zero.
// MASKED (step 6 of mpc_closed_loop_traffic_event and, in rows_from_obstacles_kernel, step 7 of
// mpc_closed_loop_obstacles_event; mk = RowMask{mask [B], sel_plan [B][NDISC]}): the rows of the agents with mask[b] != 0
// alone are written -- a held agent's row stays the one its plan was solved on -- and for those agents
// sel_plan[b] <- opp[b] (the thread of stage 0 writes it): what the plan about to be solved is solved against.
struct RowMask { const int *mask; int *sel_plan; };
template <bool MASKED = false, class... MK>
__global__ void __launch_bounds__(256) discs_from_plans_kernel(int B, int N, int nx, const double *__restrict__ X,
                                                               const int *__restrict__ opp, const double *__restrict__ radius,
                                                               double *__restrict__ table, MK... mk)
{
    static_assert(sizeof...(MK) == (MASKED ? 1 : 0), "the masked form takes a RowMask, the plain form nothing");
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)B * N * NDISC) return;
    const int j = (int)(t % NDISC);
    const size_t bk = t / NDISC;
    const int k = (int)(bk % N), b = (int)(bk / N);
    const int o = opp[(size_t)b * NDISC + j];
    if constexpr (MASKED) {
        const RowMask m = (mk, ...);
        if (m.mask[b] == 0) return;
        if (k == 0) m.sel_plan[(size_t)b * NDISC + j] = o;
    }
    double cx = 0.0, cy = 0.0, r = 0.0;
    if (o >= 0 && o < B) {
        const double *__restrict__ xo = X + ((size_t)o * N + k) * nx;
        cx = xo[0]; cy = xo[1]; r = radius[o];
    }
    double *out = table + t * 3;
    out[0] = cx; out[1] = cy; out[2] = r;
}

// mpc_fields_from_plans: table[b][k][j] = [cx, cy, c, s, A, kx, ky, alpha] for o = opp[b][j] -- the opponent's planned
// position X[o][k][0..1], the device sincos of its planned heading X[o][k][2], its shape[o][0..2] as an obstacle, and the
// skew shape[o][3] * (X[b][k][3] - X[o][k][3]) (the subtraction and the product each rounded on its own) -- eight zeros
// where there is no such agent (o < 0 or o >= B).  One thread per (agent, stage, source).  MASKED: as in
// discs_from_plans_kernel.
template <bool MASKED = false, class... MK>
__global__ void __launch_bounds__(256) fields_from_plans_kernel(int B, int N, int nx, const double *__restrict__ X,
                                                                const int *__restrict__ opp, const double *__restrict__ shape,
                                                                double *__restrict__ table, MK... mk)
{
#pragma clang fp contract(off)
    static_assert(sizeof...(MK) == (MASKED ? 1 : 0), "the masked form takes a RowMask, the plain form nothing");
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)B * N * NFIELD) return;
    const int j = (int)(t % NFIELD);
    const size_t bk = t / NFIELD;
    const int k = (int)(bk % N), b = (int)(bk / N);
    const int o = opp[(size_t)b * NFIELD + j];
    if constexpr (MASKED) {
        const RowMask m = (mk, ...);
        if (m.mask[b] == 0) return;
        if (k == 0) m.sel_plan[(size_t)b * NFIELD + j] = o;
    }
    double v[NFSRC] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (o >= 0 && o < B) {
        const double *__restrict__ xo = X + ((size_t)o * N + k) * nx;
        const double *__restrict__ so = shape + (size_t)o * 4;
        const SinCos sc = m_sincos(xo[2]);
        const double dv = X[((size_t)b * N + k) * nx + 3] - xo[3];
        v[0] = xo[0]; v[1] = xo[1]; v[2] = sc.c; v[3] = sc.s;
        v[4] = so[0]; v[5] = so[1]; v[6] = so[2]; v[7] = so[3] * dv;
    }
    double *out = table + t * NFSRC;
#pragma unroll
    for (int i = 0; i < NFSRC; i++) out[i] = v[i];
}

} // namespace mpc
