// mpc_solo.hpp -- the whole solve of an agent inside ONE wavefront, without returning to the host.
//
// A round of the batched path (step_kernel -> K1a -> K1b -> K1c) costs four dependent launches
// whatever the number of agents in it; once few agents are left that is pure latency (a tail round
// with a handful of requests still takes ~55 us), and the slowest agent of a batch needs hundreds of
// rounds more than the average one.  The persistent kernel below takes over when a sub-batch group has
// few running agents left (and serves small batches from the start): a wave claims a running agent,
// then loops  advance_agent -> evaluation -> advance_agent ...  until the agent is done, and claims
// the next one.  Nothing is exchanged between waves, so no grid-wide synchronisation is needed and
// every wave reaches its exit (the claim counter runs out; an agent's state machine is bounded by the
// solver's own iteration budgets, and a trip limit guards the loop besides).
//
// The evaluation inside the wave reuses the device functions of the round path with the same
// roundings -- the wave-per-request rollout (kin_wide_rollout) for the kinematic model, the
// thread-per-agent stage_forward on one lane otherwise; stage k of the horizon on lane k
// (stage_record); the adjoint recursion on one lane (adjoint_rec) -- so an agent gets the
// same bits whichever path serves it, and the host may switch on the live request counts.
// Speculative gradients: the speculative request of a round is evaluated beside the regular one, on the
// other half of the wave -- with the lane-serial rollout (Pacejka model) always (solo_dual); with the
// wave-per-request rollout (kinematic model) on the trips that carry one (solo_halves): those trips run the
// half-wave form of the rollout (kin_wide_rollout2), whose serial recursion serves both halves in the same
// instructions, and every other trip keeps the 64-lane form.  Horizons beyond half a wave issue none -- one
// that is pending when the agent arrives is consumed either way.
#pragma once
#include "mpc_eval.hpp"

namespace mpc {

constexpr int SOLO_WAVES = 1; // one wave per workgroup: nothing is shared between waves, and the dispatcher places them freely

// Two evaluations of one agent side by side in its wave (the request of the round on lanes 0 .. 31,
// the speculative gradient on lanes 32 .. 63): possible when the rollout is the lane-serial one (the
// wave-per-request kinematic rollout needs all 64 lanes) and a horizon fits half a wave.  With it the
// persistent kernel keeps the round path's speculation for free: both serial chains advance in the same
// instructions.
__host__ __device__ inline bool solo_wide(int model, int nfe) { return model == KIN && nfe == 4; }
__host__ __device__ inline bool solo_dual(int model, int nfe, int N) { return !solo_wide(model, nfe) && N <= 32; }
// The same for the wave-per-request rollout, trip by trip: a trip that carries a speculative gradient runs the half-wave
// form of the rollout (kin_wide_rollout2: the request on lanes 0 .. 31, the speculative gradient on lanes 32 .. 63), a
// trip that carries one request keeps all 64 lanes.  The iteration that consumes the gradient saves a dependent trip.
__host__ __device__ inline bool solo_halves(int model, int nfe, int N) { return solo_wide(model, nfe) && N <= 32; }

// doubles of LDS one wave needs: history copy (MC < 0), trajectory, stage records (twice when dual)
// (solo_halves: the second trajectory and record block lie ON the history copy where that is large enough -- the state
// machine fills and reads the copy inside one step, between two evaluations it holds nothing (advance_agent with
// hist_ready = false: hist_dma and hist_wait in PH_LS_INIT), and LDS is what bounds this kernel's waves per CU at the
// headline's shapes; solo_second_on_hist)
// Lookahead (Pacejka model, N <= 16, no constraints): FOUR evaluations side by side, 16 lanes each -- the one the state
// machine asked for, its speculative gradient, and candidates the state machine is going to ask for if the test it is
// about to make fails (the next line-search trial points; the prox points of the next descent-lemma doublings),
// kept in a small cache of (point -> psi, gradient) and handed back WITHOUT an evaluation trip when asked for.
// A Pacejka evaluation uses 4 lanes for the serial rollout and N for the stage records: the other lanes of the lone
// wave are idle, and the tail of a batch is one agent's chain of dependent trips (VERDICT r3 item 4,
// profiles/r03_pacejka_tail_model.txt).  psi and grad psi are functions of the point alone (m = 0), so a cached
// evaluation is THE evaluation: results, iteration and evaluation counts are those of the plain kernel
// (MPC_NO_LOOKAHEAD; tests), only trips are saved.
constexpr int LA_SLOTS = 4, LA_LANES = 16, LA_ENTRIES = 8;
__host__ __device__ inline bool solo_lookahead(int model, int nfe, int N, int m, int no_la)
{
    return model == PAC && !no_la && m == 0 && N <= LA_LANES && solo_dual(model, nfe, N);
}
struct LaSlot { const double *in; double *grad; double *psi; int live, is_g; };   // what the 16 lanes of a slot evaluate
// doubles of LDS the cache and the slot descriptors take
__host__ __device__ inline size_t la_lds_doubles(int n) { return (size_t)LA_ENTRIES * (2 * n + 2) + LA_SLOTS * 4 + 8; }

// The persistent kernel hands advance_agent a history copy that is NOT filled ahead of the step (hist_ready): the copy is
// filled, waited for and read inside PH_LS_INIT of one step, so between two steps -- during an evaluation -- it is free.
// The overlay below is sound on that condition alone; a kernel that prefetches the history across an evaluation (as
// step_kernel does) sets this to true and gets the second half's LDS behind the first half's instead.
constexpr bool SOLO_HIST_PREFETCH = false;
template <int MODEL> __host__ __device__ inline bool solo_second_on_hist(int N, int n, int M, bool hist)
{
    return !SOLO_HIST_PREFETCH && hist && (size_t)2 * M * n >= (size_t)(N + 1) * ModelDim<MODEL>::NX + (size_t)(JacRec<MODEL>::SIZE + 1) * N;
}
template <int MODEL> __host__ __device__ inline size_t solo_lds_doubles(int nfe, int N, int n, int M, bool hist, bool la = false)
{
    constexpr int NX = ModelDim<MODEL>::NX, JS = JacRec<MODEL>::SIZE;
    const size_t per = (size_t)(N + 1) * NX + (size_t)(JS + 1) * N;
    const bool second = solo_halves(MODEL, nfe, N) && !solo_second_on_hist<MODEL>(N, n, M, hist);
    return (hist ? (size_t)2 * M * n : 0) + (la ? LA_SLOTS : solo_dual(MODEL, nfe, N) || second ? 2 : 1) * per + (la ? la_lds_doubles(n) : 0);
}

// the evaluation(s) agent `a` asked for (req: REQ_GRAD or REQ_COST, plus REQ_SPEC) by its whole wave
#if MPC_DEV_STAMP == 5
struct SoloClk { long long roll = 0, recs = 0, adj = 0; };
#define SOLO_CLK_ARG , SoloClk &clk
#define SOLO_CLK_PASS , clk
#define SOLO_CLK(field, t) do { const long long now_ = __builtin_amdgcn_s_memrealtime(); clk.field += now_ - t; t = now_; } while (0)
#else
#define SOLO_CLK_ARG
#define SOLO_CLK_PASS
#define SOLO_CLK(field, t) do { } while (0)
#endif
// DS: the tables that hold stage data (the forms: table_form_ok, mpc_solver.hpp) -- lane k hands stage_record the data
// of its stage from the agent's rows, whose addresses are wave-uniform (stage_data); the rate table's u_{k-1} and u_{k+1}
// are the evaluated row's (`row`: xe, or xe2 on the speculative half)
// alt: where the second half's trajectory and record block lie (solo_halves); nullptr: behind the first half's (solo_dual)
template <int MODEL, class... DS>
__device__ __forceinline__ void solo_eval(const DevCfg &c, const Workspace &w, int a, int lane, int req,
                                          double *traj, double *rec, double *alt SOLO_CLK_ARG, const DS &...ds)
{
#if MPC_DEV_STAMP == 5
    long long tclk = __builtin_amdgcn_s_memrealtime();
#endif
    constexpr int NX = ModelDim<MODEL>::NX, JS = JacRec<MODEL>::SIZE;
    const int N = c.N, n = c.n;
    const bool wide = solo_wide(MODEL, c.nfe);                                      // uniform
    const bool halves = solo_halves(MODEL, c.nfe, N) && (req & REQ_SPEC) != 0;      // uniform: this trip carries two requests
    const bool dual = solo_dual(MODEL, c.nfe, N) || halves;
    const int half = dual ? lane >> 5 : 0, hl = dual ? lane & 31 : lane;
    const bool ch2 = half == 1;                                     // the speculative channel: xe2 -> ge2 only
    const bool live = !ch2 || (req & REQ_SPEC) != 0;
    const bool is_g = ch2 || (req & REQ_GRAD) != 0;
    const double *__restrict__ row = (ch2 ? w.xe2 : w.xe) + (size_t)a * n;
    const bool stage_lane = live && hl < N;
    const double d = stage_lane ? row[2 * hl] : 0.0, dl = stage_lane ? row[2 * hl + 1] : 0.0;
    double *const tj = half && alt ? alt : traj + (size_t)half * ((size_t)(N + 1) * NX);
    double *const rc = half && alt ? alt + (size_t)(N + 1) * NX : rec + (size_t)half * ((size_t)(JS + 1) * N);
    double x0[NX];
#pragma unroll
    for (int i = 0; i < NX; i++) x0[i] = w.x0[(size_t)a * NX + i];
    if constexpr (MODEL == KIN) {
        // (the half-wave form's exchange area: the half's record block, which is written after the rollout)
        static_assert(11 <= JS + 1, "kin_wide_rollout2's exchange area fits a record block");
        // The scalars the serial recursion reads at every step, as registers of their own: the DevCfg arrives in sixteen-
        // register tuples, this kernel spills scalar registers by the hundred, and a tuple that is live for the sake of
        // one field was reloaded whole, three times per stage, inside phase A (4 340 lane reads in the kernel against
        // 2 564 with the copies; profiles/r19_solo_dual.txt).  The values are the DevCfg's: same bits.
        DevCfg cr = c;
        asm volatile("" : "+s"(cr.h), "+s"(cr.friction), "+s"(cr.N), "+s"(cr.lf), "+s"(cr.lr));
        if (halves) kin_wide_rollout2(cr, x0, d, dl, lane, rc, tj);
        else if (wide) kin_wide_rollout(cr, x0, d, dl, lane, [=](int k, int i, double v) { tj[k * 4 + i] = v; });
    }
    if constexpr (MODEL == PAC) {
        if (hl < 4 && live) {                              // the serial recurrence on a quad of lanes (rhs_quad)
            double x[NX];
#pragma unroll
            for (int i = 0; i < NX; i++) { x[i] = x0[i]; if (hl == 0) tj[i] = x0[i]; }
            for (int k = 0; k < N; k++) {
                StageInput<PAC> u;
                prep_input(c, row[2 * k], row[2 * k + 1], u);
                stage_forward_quad(c, u, x, hl);
                if (hl == 0) {
#pragma unroll
                    for (int i = 0; i < NX; i++) tj[(k + 1) * NX + i] = x[i];
                }
            }
        }
    } else if (!wide && hl == 0 && live) {                 // the serial recurrence, as rollout_kernel runs it
        double x[NX];
#pragma unroll
        for (int i = 0; i < NX; i++) { x[i] = x0[i]; tj[i] = x0[i]; }
        for (int k = 0; k < N; k++) {
            StageInput<MODEL> u;
            prep_input(c, row[2 * k], row[2 * k + 1], u);
            stage_forward<MODEL>(c, u, x);
#pragma unroll
            for (int i = 0; i < NX; i++) tj[(k + 1) * NX + i] = x[i];
        }
    }
    __builtin_amdgcn_wave_barrier();                       // LDS is in order within a wave
    SOLO_CLK(roll, tclk);
    if (stage_lane) {
        double xs[NX], xe[NX];
#pragma unroll
        for (int i = 0; i < NX; i++) { xs[i] = tj[hl * NX + i]; xe[i] = tj[(hl + 1) * NX + i]; }
        const double *__restrict__ clp = w.cl_index ? w.cl + (size_t)w.cl_index[a] * 2 * (size_t)c.S : w.cl;
        double *const r = rc + hl;
        const auto put = [=](int f, double v) { r[f * N] = v; };
        if (is_g) stage_sens_record<MODEL>(c, xs, xe, d, dl, put);
        Geom g;
        stage_geom(c, w, clp, w.cl_index ? w.cl_index[a] : 0, xe[0], xe[1], g);
        stage_record<MODEL>(c, w, a, ch2, is_g, hl, xs, xe, d, dl, g, put, stage_data(ds, a, hl, N, row)...);
    }
    __builtin_amdgcn_wave_barrier();
    SOLO_CLK(recs, tclk);
    if constexpr (MODEL == KIN) {
        // (the kinematic adjoint by a quad of lanes: mpc_eval.hpp adjoint_rec_quad_kin -- same bits, a third of the chain)
        if (hl < 4 && live) {
            double *psi_out = ch2 ? nullptr : w.psi_direct ? w.psi_direct + a : w.rec + (size_t)a * REC + R_PSIE;   // (the speculative half: the gradient alone)
            adjoint_rec_quad_kin(c, is_g, hl, [=](int k, int f) { return rc[f * N + k]; }, psi_out,
                                 (ch2 ? w.ge2 : w.ge) + (size_t)a * n);
        }
    } else if (hl == 0 && live) adjoint_rec<MODEL>(c, w, a, ch2, is_g, [=](int k, int f) { return rc[f * N + k]; });
    SOLO_CLK(adj, tclk);
}

// ---- lookahead: the evaluation of up to four points by one wave (Pacejka), slot s = lanes 16 s .. 16 s + 15
__device__ __forceinline__ void solo_eval_la(const DevCfg &c, const Workspace &w, int a, int lane, const LaSlot *slots,
                                             double *traj, double *rec)
{
    constexpr int NX = ModelDim<PAC>::NX, JS = JacRec<PAC>::SIZE;
    const int N = c.N;
    const int sl = lane >> 4, hl = lane & 15;
    const LaSlot d = slots[sl];
    const bool live = d.live != 0, is_g = d.is_g != 0;
    const double *__restrict__ row = d.in;
    const bool stage_lane = live && hl < N;
    const double dv = stage_lane ? row[2 * hl] : 0.0, dl = stage_lane ? row[2 * hl + 1] : 0.0;
    double *const tj = traj + (size_t)sl * ((size_t)(N + 1) * NX);
    double *const rc = rec + (size_t)sl * ((size_t)(JS + 1) * N);
    double x0[NX];
#pragma unroll
    for (int i = 0; i < NX; i++) x0[i] = w.x0[(size_t)a * NX + i];
    if (hl < 4 && live) {                                  // the serial recurrence on a quad of lanes (rhs_quad)
        double x[NX];
#pragma unroll
        for (int i = 0; i < NX; i++) { x[i] = x0[i]; if (hl == 0) tj[i] = x0[i]; }
        for (int k = 0; k < N; k++) {
            StageInput<PAC> u;
            prep_input(c, row[2 * k], row[2 * k + 1], u);
            stage_forward_quad(c, u, x, hl);
            if (hl == 0) {
#pragma unroll
                for (int i = 0; i < NX; i++) tj[(k + 1) * NX + i] = x[i];
            }
        }
    }
    __builtin_amdgcn_wave_barrier();                       // LDS is in order within a wave
    if (stage_lane) {
        double xs[NX], xe[NX];
#pragma unroll
        for (int i = 0; i < NX; i++) { xs[i] = tj[hl * NX + i]; xe[i] = tj[(hl + 1) * NX + i]; }
        const double *__restrict__ clp = w.cl_index ? w.cl + (size_t)w.cl_index[a] * 2 * (size_t)c.S : w.cl;
        double *const r = rc + hl;
        const auto put = [=](int f, double v) { r[f * N] = v; };
        if (is_g) stage_sens_record<PAC>(c, xs, xe, dv, dl, put);
        Geom g;
        stage_geom(c, w, clp, w.cl_index ? w.cl_index[a] : 0, xe[0], xe[1], g);
        stage_record<PAC>(c, w, a, /*ch2 (unused: m = 0)=*/true, is_g, hl, xs, xe, dv, dl, g, put);
    }
    __builtin_amdgcn_wave_barrier();
    if (hl == 0 && live) adjoint_rec_to<PAC>(c, is_g, [=](int k, int f) { return rc[f * N + k]; }, d.psi, d.grad);
    __builtin_amdgcn_wave_barrier();
}

// the cache: LA_ENTRIES x (point[n], gradient[n]) + psi[LA_ENTRIES] + flags[LA_ENTRIES] (0 empty, 1 psi, 2 psi and gradient)
struct LaCache {
    double *pt, *gr, *psi; int *fl; int n;
    __device__ __forceinline__ LaCache(double *base, int n_) : pt(base), gr(base + (size_t)LA_ENTRIES * n_),
        psi(base + (size_t)2 * LA_ENTRIES * n_), fl((int *)(base + (size_t)2 * LA_ENTRIES * n_ + LA_ENTRIES)), n(n_) {}
    __device__ __forceinline__ void clear(int lane) { if (lane < LA_ENTRIES) fl[lane] = 0; }
    // the entry that holds the evaluation of the point whose element `lane` is v (lanes >= n: ignored), or -1; uniform
    __device__ __forceinline__ int find(int lane, double v, bool need_grad) const
    {
        for (int e = 0; e < LA_ENTRIES; e++) {
            const int f = __builtin_amdgcn_readfirstlane(fl[e]);
            if (f == 0 || (need_grad && f != 2)) continue;
            const bool eq = lane >= n || __double_as_longlong(pt[(size_t)e * n + lane]) == __double_as_longlong(v);
            if (__ballot(!eq) == 0ull) return e;
        }
        return -1;
    }
};

// list of the agents of this view that are still running (phase != PH_DONE), in agent order inside a
// workgroup; also resets the claim counter's companion (the number of entries)
__global__ void __launch_bounds__(256) solo_list_kernel(const Workspace w, int *__restrict__ list, int *__restrict__ ctr)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = a < w.B && rec_int_of(w.rec[(size_t)a * REC + R_PHASE]) != PH_DONE;
    const unsigned long long bal = __ballot(on);
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0 && bal != 0ull) base = atomicAdd(&ctr[1], __popcll(bal));
    base = __builtin_amdgcn_readfirstlane(base);
    if (on) list[base + __popcll(bal & ((1ull << lane) - 1ull))] = a;
}

// K1 alone through the wave-per-agent evaluation (standalone entry point, parity tests): agent = block
// (want_grad bit 1: "two points, one trip" -- the speculative gradient xe2 -> ge2 rides beside the request, as on a trip
// of the persistent kernel that carries REQ_SPEC; the host asks for it where solo_halves holds)
template <int MODEL, bool PA = false, class... CT>
__global__ void __launch_bounds__(64, 1) solo_eval_kernel(const DevCfg c_, const WsArg<PA> w, int want_grad, CT... ct)
{
    static_assert(sizeof...(CT) == 0 || PA, "the constraint form exists in the per-agent-parameter form alone");
    extern __shared__ double s_solo[];
    // (PA: the agent's row is wave-uniform -- scalar loads into the private DevCfg: agent_cfg_uniform; CT: and its
    // constraint row, the same way)
    DevCfg cm_;
    if constexpr (PA) { cm_ = c_; agent_cfg_uniform(cm_, w.ptab, w.pidx, blockIdx.x); }
    static_assert(table_form_ok<CT...>(), MPC_TABLE_FORMS);
    if constexpr (has_tab<ConTab, CT...>) agent_con_uniform(cm_, ct..., blockIdx.x);
    const DevCfg &c = PA ? cm_ : c_;
    double *traj = s_solo;
    double *rec = traj + (size_t)(c.N + 1) * ModelDim<MODEL>::NX;
    double *alt = nullptr;
    if (solo_halves(MODEL, c.nfe, c.N)) alt = rec + (size_t)(JacRec<MODEL>::SIZE + 1) * c.N;
    const int ereq = ((want_grad & 1) ? REQ_GRAD : REQ_COST) | ((want_grad & 2) ? REQ_SPEC : 0);
#if MPC_DEV_STAMP == 5
    SoloClk clk;
#endif
    if constexpr (has_tab<ConTab, CT...>) solo_eval<MODEL>(c, w, blockIdx.x, threadIdx.x, ereq, traj, rec, alt SOLO_CLK_PASS);   // (it is in c)
    else
    solo_eval<MODEL>(c, w, blockIdx.x, threadIdx.x, ereq, traj, rec, alt SOLO_CLK_PASS, ct...);
}

// One agent's solve with the lookahead (Pacejka, NE = 1): the loop of solo_kernel with a cache lookup before every
// evaluation trip and candidates riding in the free slots of the trip.
// (cm: the DevCfg the evaluations run on -- c itself, or the agent's private one when a parameter table is bound;
// bx: the box the state machine and the candidate points project onto -- the DevCfg's, or the agent's own)
template <int MC, class BOX>
__device__ __forceinline__ void solo_agent_la(const DevCfg &c, const DevCfg &cm, const Workspace &w, int a, int lane, double *hist,
                                              double *traj, double *rec, double *la_base, long long max_trips, const BOX &bx)
{
#pragma clang fp contract(off)   // the candidate points are formed by the state machine's own functions: same roundings
    const int n = c.n, par = lane & 1;
    const size_t an = (size_t)a * n;
    LaCache cache(la_base, n);
    LaSlot *slots = (LaSlot *)(la_base + (size_t)LA_ENTRIES * (2 * n + 2));
    static_assert(sizeof(LaSlot) == 4 * sizeof(double), "slot descriptor layout");
    cache.clear(lane);
    int next_e = 0;                                       // round-robin replacement (uniform)
    double la_evals = 0.0, la_hits = 0.0;
    __builtin_amdgcn_wave_barrier();
    const auto ldv = [&](const double *rowp) { return lane < n ? rowp[lane] : 0.0; };
    for (long long trip = 0; trip < max_trips; trip++) {
        const AgentIn<1> in = load_agent<1>(c, w, a, lane);
        int req = advance_agent<1, MC, true, false, BOX>(c, w, a, lane, in, hist, false, /*allow_spec=*/true, false, 1 << 30, bx);
        if ((req & (REQ_GRAD | REQ_COST)) == 0) break;                // uniform: the agent is done
        // the record as the state machine left it (same wave, same addresses: ordered behind its stores)
        double rv = w.rec[(size_t)a * REC + lane];
        const int ph = __builtin_amdgcn_readlane(__double2loint(rv), R_PHASE) & PH_MASK;
        const double gam = rdlane(rv, R_GAMMA), gamn = rdlane(rv, R_GAMMAN), tau = rdlane(rv, R_TAU);
        const double Lk = rdlane(rv, R_L), Ln = rdlane(rv, R_LN);
        const bool want_g = (req & REQ_GRAD) != 0;
        bool need_main = true, need_spec = (req & REQ_SPEC) != 0;
        // ---- a descent-lemma loop that has doubled twice already: the speculative gradient of every further level
        // would be thrown away but the last one's; it is dropped (the next iteration asks for its Hessian-vector
        // gradient itself: same bits, same counted evaluations) and the slots go to deeper levels
        const bool dl_loop = (ph == PH_W_LS_C && Ln >= 4.0 * Lk) || (ph == PH_W_DL && rdlane(rv, R_GAMMA) < rdlane(rv, R_GAMMA_TOP) * 0.3);
        if (need_spec && dl_loop) {
            need_spec = false; req &= ~REQ_SPEC;
            if (lane == R_SPEC) w.rec[(size_t)a * REC + lane] = rec_int(0);
            if (lane == R_NSPEC || lane == R_NGRAD) w.rec[(size_t)a * REC + lane] = rv - 1.0;
        }
        // ---- served from the cache?
        const double xe_v = ldv(w.xe + an);
        {
            const int e = cache.find(lane, xe_v, want_g);
            if (e >= 0) {
                if (lane == 0) w.rec[(size_t)a * REC + R_PSIE] = cache.psi[e];
                if (want_g && lane < n) w.ge[an + lane] = cache.gr[(size_t)e * n + lane];
                need_main = false;
            }
        }
        if (need_spec) {
            const int e = cache.find(lane, ldv(w.xe2 + an), true);
            if (e >= 0) {
                if (lane < n) w.ge2[an + lane] = cache.gr[(size_t)e * n + lane];
                need_spec = false;
            }
        }
        if (!need_main && !need_spec) { la_hits += 1.0; continue; }   // no trip
        // ---- the slots of this trip
        int nslot = 0;
        const auto set_slot = [&](int s, const double *inp, double *g, double *ps, bool isg) {
            if (lane == 0) { slots[s].in = inp; slots[s].grad = g; slots[s].psi = ps; slots[s].live = 1; slots[s].is_g = isg ? 1 : 0; }
        };
        if (lane < LA_SLOTS) slots[lane].live = 0;
        __builtin_amdgcn_wave_barrier();
        if (need_main) set_slot(nslot++, w.xe + an, w.ge + an, w.rec + (size_t)a * REC + R_PSIE, want_g);
        if (need_spec) set_slot(nslot++, w.xe2 + an, w.ge2 + an, nullptr, true);
        // a candidate: the point (element `lane` = v) goes into a cache entry unless the cache holds it already
        int cand_e[LA_SLOTS], cand_g[LA_SLOTS], ncand = 0;
        const auto add_candidate = [&](double v, bool isg) {
            if (nslot >= LA_SLOTS) return;
            if (__ballot(lane < n && !isfinite(v)) != 0ull) return;       // (uniform) nothing to learn from a lost point
            if (cache.find(lane, v, isg) >= 0) return;
            if (__ballot(lane < n && __double_as_longlong(v) != __double_as_longlong(xe_v)) == 0ull && need_main && (want_g || !isg)) return;
            const int e = next_e; next_e = (next_e + 1) % LA_ENTRIES;
            if (lane == 0) cache.fl[e] = 0;
            if (lane < n) cache.pt[(size_t)e * n + lane] = v;
            set_slot(nslot++, cache.pt + (size_t)e * n, cache.gr + (size_t)e * n, cache.psi + e, isg);
            cand_e[ncand] = e; cand_g[ncand] = isg ? 1 : 0; ncand++;
        };
        Row<1> X, G, Q, XN, GE;
        if (ph == PH_W_LS_G) {
            // waiting for the gradient at the trial point of step tau: the next trials are tau / 2, tau / 4, tau / 8
            // while they are >= tau_min (PH_W_LS_C), the last of them the safe prox step (PH_LS_TRIAL)
            X.v[0] = ldv(w.xk + an); G.v[0] = ldv(w.gk + an); Q.v[0] = ldv(w.q + an);
            double t = tau;
            for (int j = 0; j < 3; j++) {
                t = t / 2.0;
                if (!(t >= c.tau_min)) break;
                const Row<1> xt = trial_point<1>(c, bx, par, X, G, Q, gam, t, t / 2.0 < c.tau_min);
                add_candidate(xt.v[0], true);
            }
        } else if (ph == PH_W_LS_C || ph == PH_W_DL) {
            // waiting for the cost at a prox point xhat(gamma_n) of (x, g) = the trial point and its gradient (W_LS_C) or
            // the iterate (W_DL).  If the descent lemma fails there the step is halved: xhat(gamma_n / 2), / 4, ...
            const bool at_trial = ph == PH_W_LS_C;
            XN.v[0] = ldv((at_trial ? w.xn : w.xk) + an); GE.v[0] = ldv((at_trial ? w.ge : w.gk) + an);
            const double g0 = at_trial ? gamn : gam;
            const double Lcur = at_trial ? Ln : Lk;
            if (!dl_loop && at_trial) {
                // not in a doubling loop: the next trial's cost and speculative gradient, if its gradient is known
                const double t = tau / 2.0;
                if (t >= c.tau_min) {
                    X.v[0] = ldv(w.xk + an); G.v[0] = ldv(w.gk + an); Q.v[0] = ldv(w.q + an);
                    const Row<1> xt = trial_point<1>(c, bx, par, X, G, Q, gam, t, t / 2.0 < c.tau_min);
                    const int e = cache.find(lane, xt.v[0], true);
                    if (e >= 0) {
                        Row<1> gt; gt.v[0] = lane < n ? cache.gr[(size_t)e * n + lane] : 0.0;
                        const double xh = xt.v[0] + prox_p(c, bx, par, xt.v[0], gt.v[0], gam);       // prox_to_xe at the next trial
                        add_candidate(xh, false);
                        Row<1> sp; sp.v[0] = 0.0;
                        const int nj = spec_point<1>(c, bx, par, n, lane, xt, gt, gam, sp);
                        if (!c.no_spec && nj > 0 && nj < n) add_candidate(sp.v[0], true);
                    }
                }
            }
            // deeper levels of this point's descent-lemma loop fill what is left
            double gd = g0, Ld = Lcur;
            for (int j = 0; j < LA_SLOTS; j++) {
                if (nslot >= LA_SLOTS || !(Ld * 2.0 <= c.L_max)) break;
                gd = gd / 2.0; Ld = Ld * 2.0;
                add_candidate(XN.v[0] + prox_p(c, bx, par, XN.v[0], GE.v[0], gd), false);
            }
        }
        __builtin_amdgcn_wave_barrier();
        solo_eval_la(cm, w, a, lane, slots, traj, rec);
        for (int j = 0; j < ncand; j++) if (lane == 0) cache.fl[cand_e[j]] = cand_g[j] ? 2 : 1;
        la_evals += (double)ncand;
        __builtin_amdgcn_wave_barrier();
    }
    // the lookahead's statistics of this agent (plain double counters of the record)
    if (lane == R_LA_EVALS) w.rec[(size_t)a * REC + lane] += la_evals;
    if (lane == R_LA_HITS) w.rec[(size_t)a * REC + lane] += la_hits;
}

// ctr[0] = claim counter, ctr[1] = number of list entries (list == nullptr: every agent of the view)
// Waves per SIMD the kernel is compiled for.  The kinematic variant needs 346 registers; held to 256 (two
// waves per SIMD) it spills ~90 of them and a lone wave is no slower for it (1 024 agents: 32.5 vs 33.1 ms),
// while twice as many agents are in flight (4 096 agents: 78 -> 53 ms).  The Pacejka variant needs all 512
// and its long serial chains lose more to the spills than they gain (65 536 agents: 0.97 -> 1.01 s): one wave.
#ifndef MPC_SOLO_WPS_KIN
#define MPC_SOLO_WPS_KIN 2
#endif
template <int MODEL> struct SoloOcc { static constexpr int WPS = MODEL == KIN ? MPC_SOLO_WPS_KIN : 1; };

// LA: the lookahead variant (host: solo_lookahead) -- a kernel of its own, so that neither holds the other's code
// PA: the per-agent variant (a parameter table is bound): the evaluations of agent a run on the handle's DevCfg with
// the fields of a's row, read by scalar loads when the wave claims the agent; the state machine keeps the handle's
// BT: empty, or the bounds table (one trailing BoxTab argument: mpc_set_agent_bounds) -- the agent's box is read in the
// same place, its row by scalar loads and this lane's two values of it chosen once per agent (lane_box_uniform); the state
// machine and the lookahead's candidate points project onto it.  The box form exists together with PA alone: without a
// parameter table of the caller's the host binds a one-row table of the handle's own values (mpc_launch.hpp).
// BT = (BoxTab, one of the table forms: table_form_ok, mpc_solver.hpp) -- a form exists together with the box form alone
// (the host supplies a one-row box table of the handle's own values when the caller bound none) and never with the
// lookahead, which is an unconstrained problem's and changes no result.  The constraint form: the evaluations' DevCfg
// takes the agent's constraint row with its parameter row, and the state machine projects the multipliers with the row's
// bounds (RowCon).  Every other table goes on to the evaluations (solo_eval) and leaves the state machine what it is; on a
// disc handle it projects the multipliers with the handle's bounds [0, +inf), the same for every agent.
template <int MODEL, int NE, int MC, bool LA = false, bool PA = false, class... BT>
__global__ void __launch_bounds__(64 * SOLO_WAVES, SoloOcc<MODEL>::WPS)
solo_kernel(const DevCfg c, const WsArg<PA> w, const int *__restrict__ list, int *__restrict__ ctr,
            long long max_trips, BT... bt)
{
    constexpr bool BA = has_tab<BoxTab, BT...>, CA = has_tab<ConTab, BT...>;
    static_assert(!BA || PA, "the box form of the persistent kernel exists in the per-agent-parameter form alone");
    static_assert(table_form_ok<BT...>() && (BA || sizeof...(BT) == 0), MPC_TABLE_FORMS ", behind the BoxTab");
    static_assert(!LA || sizeof...(BT) <= 1, "the lookahead is an unconstrained problem's: it has no table form but the box form");
    using BOX = BoxOf<BA, LaneBox>;
    using CON = ConOf<CA, RowCon>;
    extern __shared__ double s_solo[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t per_wave = solo_lds_doubles<MODEL>(c.nfe, c.N, c.n, c.M, MC < 0);
    const bool spec = solo_dual(MODEL, c.nfe, c.N) || solo_halves(MODEL, c.nfe, c.N);   // speculative gradients only where they ride along
    double *hist = s_solo + (size_t)wv * per_wave;
    double *traj = hist + (MC < 0 ? (size_t)2 * c.M * c.n : 0);
    double *rec = traj + (size_t)(c.N + 1) * ModelDim<MODEL>::NX;
    // the second half's trajectory and records (solo_halves): on the history copy, idle between two steps of the state
    // machine, where it is large enough (solo_second_on_hist), else behind the first half's
    double *alt = nullptr;
    if (solo_halves(MODEL, c.nfe, c.N))
        alt = solo_second_on_hist<MODEL>(c.N, c.n, c.M, MC < 0) ? hist : rec + (size_t)(JacRec<MODEL>::SIZE + 1) * c.N;
    const int total = list ? ctr[1] : w.B;
    if constexpr (LA) {
        // (one element per lane, one wave per workgroup; four trajectories, then four record blocks, then the cache)
        static_assert(!LA || (MODEL == PAC && NE == 1 && SOLO_WAVES == 1), "lookahead: Pacejka, n <= 64, one wave per workgroup");
        constexpr int NXm = ModelDim<MODEL>::NX, JSm = JacRec<MODEL>::SIZE;
        rec = traj + (size_t)LA_SLOTS * ((size_t)(c.N + 1) * NXm);
        double *la_base = rec + (size_t)LA_SLOTS * ((size_t)(JSm + 1) * c.N);
        for (;;) {
            int i = 0;
            if (lane == 0) i = atomicAdd(&ctr[0], 1);
            i = __builtin_amdgcn_readfirstlane(i);
            if (i >= total) break;
            const int a = list ? list[i] : i;
            if constexpr (BA) {
                DevCfg cm = c;
                agent_cfg_uniform(cm, w.ptab, w.pidx, a);
                solo_agent_la<MC>(c, cm, w, a, lane, hist, traj, rec, la_base, max_trips, lane_box_uniform(pack_get<BoxTab>(bt...), a, lane));
            } else if constexpr (PA) {
                DevCfg cm = c;
                agent_cfg_uniform(cm, w.ptab, w.pidx, a);
                solo_agent_la<MC>(c, cm, w, a, lane, hist, traj, rec, la_base, max_trips, CfgBox());
            } else
            solo_agent_la<MC>(c, c, w, a, lane, hist, traj, rec, la_base, max_trips, CfgBox());
        }
        return;
    }
    for (;;) {
        int i = 0;
        if (lane == 0) i = atomicAdd(&ctr[0], 1);
        i = __builtin_amdgcn_readfirstlane(i);
        if (i >= total) break;
        const int a = list ? list[i] : i;
        DevCfg cm_;
        if constexpr (PA) { cm_ = c; agent_cfg_uniform(cm_, w.ptab, w.pidx, a); }
        const DevCfg &cm = PA ? cm_ : c;
        BOX bx{};
        if constexpr (BA) bx = lane_box_uniform(pack_get<BoxTab>(bt...), a, lane);
        CON cn{};
        if constexpr (CA) {
            const ConTab &ct = pack_get<ConTab>(bt...);
            agent_con_uniform(cm_, ct.ctab, ct.cidx, a);
            cn = row_con_uniform(ct, a);
        }
#if MPC_DEV_STAMP == 5
        const long long st0 = __builtin_amdgcn_s_memrealtime();
        long long ntrip = 0, t_adv = 0, nhess = 0;   // nhess: trips that are the Hessian-vector gradient of PH_AFTER_DL alone
        SoloClk clk;
#endif
        for (long long trip = 0; trip < max_trips; trip++) {
#if MPC_DEV_STAMP == 5
            const long long ta = __builtin_amdgcn_s_memrealtime();
#endif
            const AgentIn<NE> in = load_agent<NE>(c, w, a, lane);
            const int req = advance_agent<NE, MC, true, false, BOX, CON, /*PRED=*/false>(c, w, a, lane, in, hist, /*hist_ready=*/SOLO_HIST_PREFETCH, /*allow_spec=*/spec, false, 1 << 30, bx, cn);
            if ((req & (REQ_GRAD | REQ_COST)) == 0) break;              // uniform: the agent is done
#if MPC_DEV_STAMP == 5
            t_adv += __builtin_amdgcn_s_memrealtime() - ta;
            if ((req & (REQ_GRAD | REQ_COST | REQ_SPEC)) == REQ_GRAD && (rec_int_of(w.rec[(size_t)a * REC + R_PHASE]) & PH_MASK) == PH_W_HESS) nhess++;
            ntrip++;
#endif
            // (the ladder stays here: handing solo_eval the tables behind the BoxTab through a forwarding overload, or the
            // whole pack, changes the instruction streams of this kernel's forms -- profiles/r24_stage_data.txt)
            constexpr bool DA = has_tab<DiscTab, BT...>, RA = has_tab<RateTab, BT...>, FA = has_tab<FieldTab, BT...>, WA = has_tab<RoadTab, BT...>;
            if constexpr (WA && FA) solo_eval<MODEL>(cm, w, a, lane, req, traj, rec, alt SOLO_CLK_PASS, pack_get<RateTab>(bt...), pack_get<FieldTab>(bt...), pack_get<RoadTab>(bt...));
            else if constexpr (WA) solo_eval<MODEL>(cm, w, a, lane, req, traj, rec, alt SOLO_CLK_PASS, pack_get<DiscTab>(bt...), pack_get<RateTab>(bt...), pack_get<RoadTab>(bt...));
            else if constexpr (FA) solo_eval<MODEL>(cm, w, a, lane, req, traj, rec, alt SOLO_CLK_PASS, pack_get<RateTab>(bt...), pack_get<FieldTab>(bt...));
            else if constexpr (DA && RA) solo_eval<MODEL>(cm, w, a, lane, req, traj, rec, alt SOLO_CLK_PASS, pack_get<DiscTab>(bt...), pack_get<RateTab>(bt...));
            else if constexpr (RA) solo_eval<MODEL>(cm, w, a, lane, req, traj, rec, alt SOLO_CLK_PASS, pack_get<RateTab>(bt...));
            else if constexpr (DA) solo_eval<MODEL>(cm, w, a, lane, req, traj, rec, alt SOLO_CLK_PASS, pack_get<DiscTab>(bt...));
            else
            solo_eval<MODEL>(cm, w, a, lane, req, traj, rec, alt SOLO_CLK_PASS);
        }
#if MPC_DEV_STAMP == 5
        if (lane == 0 && i < DEV_STAMPS) {   // (one buffer for all groups: the claim index of the group whose kernel ran last wins)
            g_dev_stamps[4 * i] = st0; g_dev_stamps[4 * i + 1] = __builtin_amdgcn_s_memrealtime();
            g_dev_stamps[4 * i + 2] = ntrip | (t_adv << 20); g_dev_stamps[4 * i + 3] = a | (clk.roll << 20);
            if (i + 32768 < DEV_STAMPS) { g_dev_stamps[4 * (i + 32768)] = clk.recs; g_dev_stamps[4 * (i + 32768) + 1] = clk.adj; g_dev_stamps[4 * (i + 32768) + 2] = nhess; }
        }
#endif
    }
}

} // namespace mpc
