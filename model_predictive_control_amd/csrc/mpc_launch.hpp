// mpc_launch.hpp -- host side of libmpc_hip.so, part 2: from the handle's run-time state to ONE instantiation of each
// kernel template.  Every run-time choice becomes template arguments in one place: a flag in with_flag, the model in
// with_model / with_model_table, the L-BFGS history variant in with_hist_variant, and the per-agent tables a kernel takes
// as its pack in with_table_form -- the one list of the table forms that exist -- and, for the step kernel, which reads
// the box and the constraint data and no other table, in with_step_form.  So each kernel template is named at one launch
// site, and a new flag or table is added once.  What is instantiated is what these functions and the `if constexpr`s
// below let through, never the cross product: the Pacejka model has no fused K1b + K1c, the lookahead exists for
// <PAC, NE = 1> without a table form alone, adjoint_kernel has no per-agent form, and the step kernel has a constraint
// form on a constrained problem alone.
#pragma once
#include "mpc_handle.hpp"

#include <type_traits>

template <int V> using int_c = std::integral_constant<int, V>;
// f(std::true_type / std::false_type) for a run-time flag
template <class F> static void with_flag(bool b, F &&f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
// f(int_c<KIN> / int_c<PAC>) for the handle's model; returns what f returns
template <class F> static auto with_model(int model, F &&f) { if (model == PAC) return f(int_c<PAC>{}); return f(int_c<KIN>{}); }
// The standalone kernels (mpc_aux.hpp, solo_eval_kernel) for this handle's model, with or without the bound parameter
// table: f(MODEL, PA, pt...) where pt is the kernels' trailing pack -- (table, index) when a table is bound, empty when
// none is.  `index` is the controller's row per agent, or the plant's (mpc_closed_loop).
template <class F> static void with_model_table(const mpc_handle *h, const int32_t *index, F &&f)
{
    with_model(h->dc.model, [&](auto MODEL) {
        if (h->params().table) f(MODEL, std::true_type{}, h->params().table, index);
        else f(MODEL, std::false_type{});
    });
}

// The workspace as every kernel form with a table argument takes it: those forms exist together with the parameter form
// alone (PA = true), so without a parameter table of the caller's they run on the handle's own one-row table
// (mpc_handle::own; its index of zeros needs no slicing per group)
static WorkspacePA with_own_params(const mpc_handle *h, const WorkspaceHost &w)
{
    WorkspacePA wp = w;
    if (!wp.ptab) { wp.ptab = h->own.ptab; wp.pidx = h->own.pidx; }
    return wp;
}
// ... and the box as the table forms of the persistent kernel take it: they exist behind the box form alone, so
// without a bounds table of the caller's they run on the handle's own one-row box table (OwnTables::btab)
static BoxTab with_own_box(const mpc_handle *h, const WorkspaceHost &w) { return w.bound(TAB_BOX) ? w.box() : BoxTab{h->own.btab, h->own.pidx}; }

// The table forms of stage_kernel, stage_adjoint_kernel, solo_eval_kernel and (behind BoxTab) solo_kernel: which tables
// view `w` hands its kernels as their trailing pack t..., decided by what is bound, the first that applies:
//   1. a road table         on a disc handle <DiscTab, RateTab, RoadTab>, elsewhere <RateTab, FieldTab, RoadTab>
//   2. a constraint table   <ConTab>
//   3. a field table        <RateTab, FieldTab>
//   4. a rate table         beside a disc table <DiscTab, RateTab>, else <RateTab>
//   5. a disc table         <DiscTab>                                  (a handle of MPC_CONSTR_DISCS)
//   6. none of them         the empty pack: the kernels without a table argument
// (bind_agent_table refuses the pairs no form takes).  A form that stands behind a table the caller has not bound runs on
// the handle's own one-row table of zeros in its place (`rates`: OwnTables::rtab, zero weights; `fields`:
// OwnTables::ftab, A == 0 is skipped by a branch -- neither changes a bit).  f(PA, wp, t...): a table form is a form
// of the per-agent kernel (PA = std::true_type, wp = with_own_params), the empty pack keeps the run-time choice (PA says
// whether a parameter table is bound, wp = w) -- so naming kernel<..., PA(), decltype(t)...> instantiates these forms alone.
template <class F> static void with_table_form(const mpc_handle *h, const WorkspaceHost &w, F &&f)
{
    const auto rates = [&] { return w.bound(TAB_RATES) ? w.rate() : RateTab{h->own.rtab, h->own.pidx}; };
    const auto fields = [&] { return w.bound(TAB_FIELDS) ? w.field() : FieldTab{h->own.ftab, h->own.pidx}; };
    const auto form = [&](auto... t) { f(std::true_type{}, with_own_params(h, w), t...); };
    const bool discs = w.bound(TAB_DISCS);
    if (w.bound(TAB_ROADS)) { if (discs) form(w.disc(), rates(), w.road()); else form(rates(), fields(), w.road()); }
    else if (w.bound(TAB_CONSTR)) form(w.con());
    else if (w.bound(TAB_FIELDS)) form(rates(), w.field());
    else if (w.bound(TAB_RATES)) { if (discs) form(w.disc(), w.rate()); else form(w.rate()); }
    else if (discs) form(w.disc());
    else with_flag(w.ptab != nullptr, [&](auto PA) { f(PA, WorkspacePA(w)); });
}

// The forms of step_kernel, the one kernel of the round path that reads the box and the constraint data: f(HASM, t...)
// with the tables view `w` hands it as its pack -- the bounds table and the constraint table where they are bound, the
// box first (the same list on the device: step_form_ok).  A constraint table is bound on a constrained problem or it
// would not be, so its forms exist for HASM = true alone.
template <class F> static void with_step_form(const mpc_handle *h, const WorkspaceHost &w, F &&f)
{
    const auto form = [&](auto HASM, auto... t) { if (w.bound(TAB_BOX)) f(HASM, w.box(), t...); else f(HASM, t...); };
    if (w.bound(TAB_CONSTR)) form(std::true_type{}, w.con());
    else with_flag(h->dc.m != 0, [&](auto HASM) { form(HASM); });
}

// How the step kernel and the persistent kernel read an agent's L-BFGS history -- f(int_c<NE>, int_c<MC>), the two
// kernels' template arguments (results do not depend on the choice).  NE: elements per lane, 1 up to n = 64 and 2
// beyond.  MC < 0: through an LDS copy (one element per lane: up to M n = 800, 12.5 KiB per wave); MC = 0: from global
// memory (a longer history, or MPC_STEP_REGS).  The two kernels differ at n > 64, and this is the one place that says
// so: the step kernel (SOLO = false) has an LDS copy there too, <2, -1>, whatever M is (step_lds_pairs sizes it);
// the persistent kernel (SOLO = true) has <2, 0> alone.
template <bool SOLO, class F> static void with_hist_variant(int n, int M, bool step_regs, F &&f)
{
    if (n <= 64) with_flag(!step_regs && M * n <= 800, [&](auto LDS) { f(int_c<1>{}, int_c<LDS() ? -1 : 0>{}); });
    else if constexpr (SOLO) f(int_c<2>{}, int_c<0>{});
    else with_flag(!step_regs, [&](auto LDS) { f(int_c<2>{}, int_c<LDS() ? -1 : 0>{}); });
}

// returns true when K1b and K1c ran as one launch
template <int MODEL>
static bool launch_eval_t(mpc_handle *h, const WorkspaceHost &w, hipStream_t s, const int *lists, const int *counts,
                          int nG, int nC, hipEvent_t eva, hipEvent_t evb, int slot_bound, int *desc)
{
    const DevCfg &c = h->dc;
    const bool shared = w.cl_index == nullptr;
    const bool pa = w.ptab != nullptr;   // a parameter table is bound: the per-agent instantiation of every K1 kernel
    // list mode: the grid covers the most requests the round can hold -- every agent on both lists
    // (cost + speculative gradient), or the caller's tighter bound (blocks beyond the lists exit at once,
    // but late in a solve dispatching thousands of them costs more than the work)
    int nblk = counts ? 2 * (w.Bp / 64) : ((nG + 63) / 64 + (nC + 63) / 64);
    if (counts && slot_bound >= 0) nblk = std::min(nblk, (slot_bound + 126) / 64 + 1);
    if (nblk == 0) return true;
    const size_t lds = sizeof(double) * 64 * (size_t)(c.n + 1) + 64 * sizeof(int);
    // Kinematic model.  Few requests (late rounds of a solve, small batches): one wave per request, see
    // rollout_wide_kernel.  Otherwise two lanes per request (rollout_pair_kernel); the wave-per-request kernel keeps
    // the rounds with few requests (its wave-wide redo of a request: kin_wide_rollout).
    // Pacejka model.  Four lanes per request while a round holds few requests (a shorter chain per request where waves
    // are alone on their SIMDs); one thread per request -- 2.2 times fewer instructions in all -- once the launch fills
    // the chip (pac_quad_max: requests bound up to which the four-lane kernel runs; since the lost stages are parked no
    // request drags its wave, and the full rounds are bound by what they execute: profiles/r03_experiments.txt 34)
    const bool wide = MODEL == KIN && counts && slot_bound >= 0 && slot_bound <= h->wide_max && c.nfe == 4 && c.N <= 64;
    const bool quad = MODEL == KIN ? !wide && h->quad_rollout && c.nfe == 4 && c.N <= 64
                                   : h->quad_rollout && !(counts && slot_bound >= 0 && slot_bound > h->pac_quad_max);
    with_flag(pa, [&](auto PA) {
        if constexpr (MODEL == KIN) {
            if (wide)
                hipLaunchKernelGGL(rollout_wide_kernel<PA()>, dim3((unsigned)(nblk * 16)), dim3(256), 0, s, c, w, lists, counts);
            else if (quad)
                hipLaunchKernelGGL(rollout_pair_kernel<PA()>, dim3((unsigned)(nblk * 2)), dim3(64),
                                   sizeof(double) * 32 * (size_t)(c.n + 1), s, c, w, lists, counts, nG, nC);
        } else if (quad)
            hipLaunchKernelGGL(rollout_quad_kernel<PA()>, dim3((unsigned)(nblk * 4)), dim3(64),
                               sizeof(double) * 16 * (size_t)(c.n + 1), s, c, w, lists, counts, nG, nC);
        if (!wide && !quad)
            hipLaunchKernelGGL((rollout_kernel<MODEL, PA()>), dim3((unsigned)nblk), dim3(64), lds, s, c, w, lists, counts, nG, nC);
    });
    if (eva) (void)hipEventRecord(eva, s);
    // (kinematic model only: the Pacejka stage needs more registers than the fused kernel leaves it)
    if constexpr (MODEL == KIN) {
        if (h->fused_eval && (!counts || (slot_bound >= 0 && slot_bound <= h->fused_max))) {
            // K1b + K1c in one launch, stage records through LDS (see stage_adjoint_kernel)
            constexpr int JS = JacRec<MODEL>::SIZE;
            const int spb = FUSED_BLK / c.N;
            const int gb = (nblk * 64 + spb - 1) / spb;
            const size_t flds = sizeof(double) * (size_t)(JS + 1) * c.N * spb;
            with_table_form(h, w, [&](auto PA, const WorkspacePA &wp, auto... t) { with_flag(shared, [&](auto SH) {
                hipLaunchKernelGGL((stage_adjoint_kernel<MODEL, SH(), PA(), decltype(t)...>), dim3((unsigned)gb), dim3(FUSED_BLK), flds, s, c,
                                   wp, counts, nG, nC, desc, t...);
            }); });
            if (evb) (void)hipEventRecord(evb, s);
            return true;
        }
    }
    // (tried: nblk rounded up to a multiple of 8, which puts every stage block of slot block sb and its adjoint
    // block on XCD sb % 8 so that K1c could read records from the L2 they were written to -- no change: the 13 MB
    // of records per XCD and launch pass through a 4 MB L2 long before K1c starts)
    const size_t xy_lds = (shared && w.near.gmeta && c.S <= GRID_LDS_MAX_S) ? sizeof(double) * 2 * (size_t)c.S : 0;
    with_table_form(h, w, [&](auto PA, const WorkspacePA &wp, auto... t) { with_flag(shared, [&](auto SH) {
        hipLaunchKernelGGL((stage_kernel<MODEL, SH(), PA(), decltype(t)...>), dim3((unsigned)(nblk * c.N)), dim3(64), xy_lds, s, c,
                           wp, counts, nG, nC, nblk, t...);
    }); });
    if (evb) (void)hipEventRecord(evb, s);
    hipLaunchKernelGGL((adjoint_kernel<MODEL>), dim3((unsigned)nblk), dim3(64), 0, s, c, w, counts, nG, nC, desc);
    return false;
}
static bool launch_eval(mpc_handle *h, const WorkspaceHost &w, hipStream_t s, const int *lists, const int *counts, int nG, int nC,
                        hipEvent_t eva = nullptr, hipEvent_t evb = nullptr, int slot_bound = -1, int *desc = nullptr)
{
    return with_model(h->dc.model, [&](auto MODEL) { return launch_eval_t<MODEL()>(h, w, s, lists, counts, nG, nC, eva, evb, slot_bound, desc); });
}

// K1 alone, one wave per agent: the evaluation as the persistent kernel runs it (mpc_solo.hpp)
static void launch_solo_eval(mpc_handle *h, const WorkspaceHost &w, hipStream_t s, int want_grad)
{
    const DevCfg &c = h->dc;
    with_model(c.model, [&](auto MODEL) { with_table_form(h, w, [&](auto PA, const WorkspacePA &wp, auto... t) {
        const size_t lds = sizeof(double) * solo_lds_doubles<MODEL()>(c.nfe, c.N, c.n, c.M, false);
        hipLaunchKernelGGL((solo_eval_kernel<MODEL(), PA(), decltype(t)...>), dim3((unsigned)w.B), dim3(64), lds, s, c, wp, want_grad, t...);
    }); });
}

// LDS copy of an agent's L-BFGS history in the step kernel (MC < 0): the ring slots 0 .. P - 1, 2 P n doubles per
// wave.  P is what lets the kernel's occupancy target (step_waves_per_simd: its workgroups per CU) share a CU's 160 KiB
// -- 12 pairs at n = 40 for five workgroups, where an application reads 5.4 on average; a longer history reads its
// remaining slots from global memory.  Two elements per lane (n > 64; BASELINE config 3: N = 40, n = 80, M = 40):
// three workgroups per CU, 10 pairs of 2 x 640 B per wave at n = 80, where an application reads 11.7 on average
// (DESIGN.md 5).  With state constraints (m > 0) the whole history.  lds_pairs > 0 (MPC_LDS_PAIRS: experiments,
// tests) overrides the choice.
static constexpr size_t CU_LDS_BYTES = 160 * 1024;
static constexpr size_t STEP_LDS_RESERVE = 1024;   // per workgroup: s_req / s_next (264 B) and the allocation granule
static int step_lds_pairs(int ne, int n, int M, int m, int lds_pairs)
{
    if (lds_pairs > 0) return std::max(1, std::min(M, lds_pairs));
    if (m != 0 && ne == 1) return M;
    const size_t per_pair = (size_t)STEP_WAVES * 2 * n * sizeof(double);
    const int fit = (int)((CU_LDS_BYTES / step_waves_per_simd(ne, -1, m != 0) - STEP_LDS_RESERVE) / per_pair);
    return std::max(1, std::min(M, fit));
}
// dynamic LDS of a step launch: the history copies of its four waves, or the chain blocks' tile if that is larger
static size_t step_dyn_lds(int ne, int n, int P, bool chain)
{
    size_t lds = (size_t)STEP_WAVES * 2 * P * n * sizeof(double);
    if (ne == 1 && chain) lds = std::max(lds, chain_lds_bytes(n));
    return lds;
}

template <int NE, int MC>
static void launch_step_t(mpc_handle *h, const WorkspaceHost &w, hipStream_t s, int *lists, int *counts, int *counts_next,
                          int slot_bound, int par)
{
    const int P = MC < 0 ? step_lds_pairs(NE, h->dc.n, h->dc.M, h->dc.m, h->lds_pairs) : h->dc.M;
    const int Pl = MC < 0 ? P : 0;
    // thread-per-agent blocks for the agents that wait in PH_W_LS_G (chain_block): one per 64 gradient slots the
    // finished round can have held (the same bound that sizes the K1 grids)
    // ... only while the round is a full one: the thread-per-agent chain is ~15 us long whatever the count, which a
    // step launch of > 100 us hides and a thin round's does not (chain_min: requests bound from which they are used)
    int nchain = 0;
    DevCfg dcl = h->dc;
    dcl.chain = h->dc.chain && slot_bound >= h->chain_min;
    // MPC_SPEC_POLICY=2: descent-lemma retries do not speculate in the launches that carry the chain blocks -- the full rounds
    // of big groups, where the round of latency it costs an agent is hidden, and only where the blocks are on at all (not
    // under MPC_NO_CHAIN, for n > 64 or, unless MPC_CHAIN_MIN is set, on the Pacejka model: no workload but the one the
    // policy was measured on gets more rounds from it)
    dcl.spec_retry = h->dc.spec_policy >= 2 && dcl.chain ? h->spec_depth : 0;
    if (NE == 1 && dcl.chain) {
        nchain = w.Bp / 64;
        if (slot_bound >= 0) nchain = std::min(nchain, (slot_bound + 126) / 64 + 1);
    }
    const size_t lds = step_dyn_lds(NE, h->dc.n, Pl, NE == 1 && dcl.chain);
    // agents per workgroup: a wave walks apb / 4 agents serially, so a smaller apb trades the work per launch of
    // a workgroup for more of them resident.  The lean variant (history in LDS, five workgroups per CU) takes 32
    // for a sub-batch group of 16 Ki - 32 Ki agents (the headline's four groups): 512 workgroups per group launch, so
    // the groups' step launches fill the fifth slot of every CU; a 64 Ki one-stream launch keeps 64 (its 1 024
    // workgroups leave the fifth slots to its chain blocks).  Measured, 65 536 kinematic agents, same box
    // (profiles/r05_experiments.txt entry 1; headline k solves/s | one-stream step kernel ms per solve):
    //   P = 15, apb 64 (four per CU): 483.8 - 485.7 | 60.0     P = 15, apb 32: 476.7 | 63.9
    //   P = 12, apb 64:  493.4 | 57.0     P = 12, apb 32:  499.0 | 62.5     P = 12, apb 16:  455.6 | 71.9
    //   P = 12, apb 32 for 16 Ki groups, 64 for 64 Ki (kept): 498.8 - 499.6 | 56.4 - 56.6
    // Pacejka (4 x 16 Ki, same kernel, all 12 pairs in LDS): apb 32 vs 64 within the spread (160.0 - 161.1 vs
    // 159.2 - 160.7 k).  Below 16 Ki (and every other variant) as measured in round 2: B = 1 Ki, 4 Ki -> 4; 8 Ki -> 16.
    const int apb_env = h->apb_env;
    const bool lean = MC < 0 && NE == 1 && h->dc.m == 0;
    const int apb = apb_env == 64 || apb_env == 32 || apb_env == 16 || apb_env == 8 || apb_env == 4 ? apb_env
                  : w.B >= 32768 ? 64 : w.B >= 16384 ? (lean ? 32 : 64) : w.B >= 6144 ? 16 : 4;
    const int nstep = (w.B + apb - 1) / apb;
    with_step_form(h, w, [&](auto HASM, auto... t) {
        hipLaunchKernelGGL((step_kernel<NE, MC, HASM(), decltype(t)...>), dim3((unsigned)(nstep + nchain)), dim3(64 * STEP_WAVES), lds,
                           s, dcl, w, t..., lists, counts, counts_next, apb, nstep, par, P);
    });
}
static void launch_step(mpc_handle *h, const WorkspaceHost &w, hipStream_t s, int *lists, int *counts, int *counts_next,
                        int slot_bound, int par)
{
    with_hist_variant<false>(h->dc.n, h->dc.M, h->step_regs, [&](auto NE, auto MC) {
        launch_step_t<NE(), MC()>(h, w, s, lists, counts, counts_next, slot_bound, par);
    });
}

// The persistent wave-per-agent kernel for the agents of view `v` that are still running (`listed`:
// a list of them is built first; otherwise every agent of the view is claimed).  `bound` = an upper
// bound on the number of agents it will find.
template <int MODEL, int NE, int MC>
static void launch_solo_t(mpc_handle *h, const WorkspaceHost &v, hipStream_t s, int *ctr, bool listed, int bound,
                          long long max_trips)
{
    const DevCfg &c = h->dc;
    int *list = listed ? v.lists : nullptr;   // the round lists are free once the group leaves the rounds
    if (listed)
        hipLaunchKernelGGL(solo_list_kernel, dim3((unsigned)((v.B + 255) / 256)), dim3(256), 0, s, v, list, ctr);
    const bool la = NE == 1 && solo_lookahead(MODEL, c.nfe, c.N, c.m, c.no_la);
    const size_t lds = sizeof(double) * SOLO_WAVES * solo_lds_doubles<MODEL>(c.nfe, c.N, c.n, c.M, MC < 0, la);
    int nblk = (bound + SOLO_WAVES - 1) / SOLO_WAVES;
    nblk = std::max(1, std::min(nblk, 4 * SoloOcc<MODEL>::WPS * h->num_cus)); // what is resident (registers); the rest queues
    // The kernel's trailing pack bt...: empty (a parameter table bound or not), <BoxTab> when a bounds table is bound, and
    // <BoxTab, t...> for every table form of with_table_form (the caller's box or the handle's own).  The lookahead
    // kernel exists where solo_lookahead can say yes -- Pacejka model, one element per lane -- and without a table form:
    // those run the kernel without it on the lookahead's LDS size (results do not depend on the lookahead).
    const auto launch = [&](auto PA, const WorkspacePA &wp, auto... bt) {
        constexpr bool HAS_LA = MODEL == PAC && NE == 1 && sizeof...(bt) <= 1;
        with_flag(la && HAS_LA, [&](auto LA) {
            if constexpr (!LA() || HAS_LA)
                hipLaunchKernelGGL((solo_kernel<MODEL, NE, MC, LA(), PA(), decltype(bt)...>), dim3((unsigned)nblk), dim3(64 * SOLO_WAVES), lds, s, c,
                                   wp, list, ctr, max_trips, bt...);
        });
    };
    with_table_form(h, v, [&](auto PA, const WorkspacePA &wp, auto... t) {
        if constexpr (sizeof...(t) != 0) launch(PA, wp, with_own_box(h, v), t...);
        else if (v.bound(TAB_BOX)) launch(std::true_type{}, with_own_params(h, v), v.box());
        else launch(PA, wp);
    });
}
static void launch_solo(mpc_handle *h, const WorkspaceHost &v, hipStream_t s, int *ctr, bool listed, int bound,
                        long long max_trips)
{
    const DevCfg &c = h->dc;
    with_model(c.model, [&](auto MODEL) { with_hist_variant<true>(c.n, c.M, h->step_regs, [&](auto NE, auto MC) {
        launch_solo_t<MODEL(), NE(), MC()>(h, v, s, ctr, listed, bound, max_trips);
    }); });
}
// the persistent kernel can run this configuration: its waves' LDS fits a workgroup's 64 KiB
static bool solo_fits(const mpc_handle *h)
{
    const DevCfg &c = h->dc;
    size_t per = 0;
    with_model(c.model, [&](auto MODEL) { with_hist_variant<true>(c.n, c.M, h->step_regs, [&](auto NE, auto MC) {
        const bool la = NE() == 1 && solo_lookahead(c.model, c.nfe, c.N, c.m, c.no_la);
        per = solo_lds_doubles<MODEL()>(c.nfe, c.N, c.n, c.M, MC() < 0, la);
    }); });
    return c.N <= 64 && per * SOLO_WAVES * sizeof(double) <= 64 * 1024;
}
