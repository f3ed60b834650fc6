// mpc_rounds.hpp -- host side of libmpc_hip.so, part 3: the round loop of a batched solve.  Sub-batch groups on streams
// of their own, two polled windows of rounds in flight per group, the hand-over to the persistent kernel, and what
// the handle reports about the solve afterwards.  Host code only; included by mpc_api.hip alone.
#pragma once
#include "mpc_launch.hpp"

// a view of the workspace restricted to agents [lo, hi): local agent ids, own lists / scratch
static WorkspaceHost group_view(const WorkspaceHost &w, const DevCfg &c, int g, int lo, int hi)
{
    WorkspaceHost v = w;
    const size_t n = c.n, m = c.m, M = c.M;
    v.x0 = w.x0 + (size_t)lo * c.nx; v.xo = w.xo + (size_t)lo * n;
    v.xk = w.xk + (size_t)lo * n; v.gk = w.gk + (size_t)lo * n; v.q = w.q + (size_t)lo * n;
    v.xn = w.xn + (size_t)lo * n; v.xe = w.xe + (size_t)lo * n; v.ge = w.ge + (size_t)lo * n;
    v.xe2 = w.xe2 + (size_t)lo * n; v.ge2 = w.ge2 + (size_t)lo * n;
    v.S = w.S + (size_t)lo * M * n; v.Y = w.Y + (size_t)lo * M * n;
    if (w.y) v.y = w.y + (size_t)lo * m;
    v.Sig = w.Sig + (size_t)lo * m; v.Sig_old = w.Sig_old + (size_t)lo * m; v.e1 = w.e1 + (size_t)lo * m;
    v.e2 = w.e2 + (size_t)lo * m; v.yhx = w.yhx + (size_t)lo * m; v.yhxn = w.yhxn + (size_t)lo * m;
    v.yhe = w.yhe + (size_t)lo * m;
    v.rec = w.rec + (size_t)lo * REC;
    if (w.cl_index) v.cl_index = w.cl_index + lo;
    if (w.pidx) v.pidx = w.pidx + lo;   // the per-agent row indices of the bound tables
    for (WorkspaceHost::Tab &t : v.tabs)
        if (t.rows) t.rows += lo;
    const size_t soff = 2 * (size_t)lo + 64 * (size_t)g; // disjoint slot intervals inside the shared scratch
    v.trajx = w.trajx + soff; v.useq = w.useq + soff; v.stage_L = w.stage_L + soff; v.jac = w.jac + soff;
    v.agent_of = w.agent_of + soff;
    v.lists = w.lists + lo;
    v.counts = w.counts + 8 * g;
    v.B = hi - lo; v.Bp = (v.B + 63) & ~63;
    return v;
}

// One solve's host state and the steps of the solve as members, in the order run() calls them (at the end).
struct SolveRun {
    mpc_handle *const h;
    const hipStream_t s;                 // the caller's stream: the solve begins and ends on it
    const DevCfg &c;
    WorkspaceHost &w;
    const int B, check_every;
    long long max_rounds = 0;
    bool solo_ok = false, all_solo = false;
    // the sub-batch groups: views of the workspace, streams, progress
    int ng = 0, nactive = 0;
    WorkspaceHost gv[MPC_MAX_GROUPS];
    hipStream_t gs[MPC_MAX_GROUPS];      // (one group: the caller's stream)
    struct GroupRun { long long round = 0, window = 0; bool active = true; int slot_bound = 0; };
    GroupRun gr[MPC_MAX_GROUPS];
    long long launch_sets = 0, unfused_sets = 0, solo_launches = 0, rounds_done[MPC_MAX_GROUPS] = {0};
    int rc_loop = MPC_OK;
    size_t nev = 0;               // profile mode: events 0 .. nev-1 of the pool, five per sampled launch set
    bool solo_timed[MPC_MAX_GROUPS] = {false};
    const bool host_trace, host_timing;         // MPC_HOST_TRACE / MPC_HOST_TIMING
    double host_queue_s = 0.0;                  // host time spent queueing launches (MPC_HOST_TIMING: printed at the end)
    long long dry_windows = 0, first_dry_round = -1;
    std::vector<std::array<long long, 4>> trace;                 // MPC_HOST_TRACE: one line per polled window
    std::chrono::steady_clock::time_point t_loop0;

    SolveRun(mpc_handle *h_, hipStream_t s_)
        : h(h_), s(s_), c(h_->dc), w(h_->ws), B(h_->ws.B), check_every(h_->check_every),
          host_trace(!h_->host_trace.empty()), host_timing(h_->host_timing) {}

    // the solver records of a fresh solve, the handle's figures back to zero, the round guard
    int begin()
    {
        HIPCHK(hipMemsetAsync(w.counts, 0, sizeof(DevCounters), s));   // counts, totals and solo_ctr
        hipLaunchKernelGGL(init_kernel, dim3((unsigned)(((size_t)B * REC + 255) / 256)), dim3(256), 0, s, c, w);
        h->rounds = 0; h->evals_grad = 0; h->evals_cost = 0; h->eval_ms = 0.0; h->step_ms = 0.0;
        h->lbfgs_ms = 0.0; h->lbfgs_rows = 0; h->solo_agents = 0;
        for (int k = 0; k < 5; k++) { h->kernel_ms[k] = 0.0; h->kernel_launches[k] = 0; }
        // Guard against a runaway loop only: a valid solve must never reach it.  An inner iteration costs at
        // most ~(4 + 11 * 60) evaluations (nine line-search trials whose quadratic-upper-bound loop doubles L
        // up to L_max), an outer iteration a handful more; with an evaluation budget an agent stops at the
        // first stop test past it.  Every running agent consumes at least one evaluation per round.
        const long long per_iter = 700;
        max_rounds = per_iter * ((long long)c.max_total_inner + 16) + 8LL * c.max_outer + 1024;
        if (c.max_total_evals > 0) max_rounds = std::min(max_rounds, (long long)c.max_total_evals + per_iter + 8LL * c.max_outer + 1024);
        if (h->round_limit > 0) max_rounds = std::min(max_rounds, h->round_limit);   // mpc_set_round_limit (test aid)
        solo_ok = (h->solo_max > 0 || h->solo_all > 0) && solo_fits(h);
        // small batch: every agent is solved by one wave of the persistent kernel from the start
        all_solo = solo_ok && B <= h->solo_all;
        return MPC_OK;
    }

    // groups: contiguous agent ranges (multiples of 64), each with its own stream; measured at
    // B = 65536 (round 1): 1 group 0.258 s, 2 groups 0.224 s, 3 groups 0.220 s per solve.  The HIP runtime
    // maps a process's streams to GPU_MAX_HW_QUEUES hardware queues (4 unless the environment says
    // otherwise): with the caller's stream that leaves three for groups -- a fourth group shares a queue with
    // another and its launches wait behind that one's (round 2: 3 groups 169.8 ms, 4 groups 259.8 ms with 4
    // queues, 165.7 ms with 8; 5 groups 196 ms).  Four groups only when the queues are there.
    int plan_groups_and_fork()
    {
        int G = h->ngroups > 0 ? h->ngroups : (B >= 49152 && h->hw_queues >= 5 ? 4 : B >= 24576 ? 3 : B >= 16384 ? 2 : 1);
        if (G > MPC_MAX_GROUPS) G = MPC_MAX_GROUPS;
        while (G > 1 && B / G < 1024) G--;
        if (all_solo) G = 1;
        const int per = (((B + G - 1) / G) + 63) & ~63;
        for (int g = 0; g < G; g++) {
            const int lo = g * per, hi = std::min(B, lo + per);
            if (lo >= hi) break;
            gv[ng] = group_view(w, c, ng, lo, hi);
            ng++;
        }
        h->groups_last = ng;
        if (ng == 1) gs[0] = s;
        else {
            if (!h->gevent[MPC_MAX_GROUPS]) HIPCHK(hipEventCreateWithFlags(&h->gevent[MPC_MAX_GROUPS], hipEventDisableTiming));
            HIPCHK(hipEventRecord(h->gevent[MPC_MAX_GROUPS], s)); // fork
            for (int g = 0; g < ng; g++) {
                if (!h->gstream[g]) HIPCHK(hipStreamCreateWithFlags(&h->gstream[g], hipStreamNonBlocking));
                if (!h->gevent[g]) HIPCHK(hipEventCreateWithFlags(&h->gevent[g], hipEventDisableTiming));
                gs[g] = h->gstream[g];
                HIPCHK(hipStreamWaitEvent(gs[g], h->gevent[MPC_MAX_GROUPS], 0));
            }
        }
        // upper bound on a group's requests per round: at most two per running agent (evaluation +
        // speculative gradient); every running agent has at least one request in a round and agents only
        // ever finish, so twice the requests seen at a poll bounds every later round
        for (int g = 0; g < ng; g++) gr[g].slot_bound = 2 * gv[g].B;
        nactive = ng;
        return MPC_OK;
    }

    // group g's agents that are still running (all of them: !listed) finish in the persistent kernel
    void hand_to_solo(int g, int *ctr, bool listed, int bound)
    {
        solo_event(g, 0);
        launch_solo(h, gv[g], gs[g], ctr, listed, bound, max_rounds);
        solo_event(g, 1);
        solo_launches++;
    }
    void solo_event(int g, int which) // profile mode: (start, stop) around the launch
    {
        if (!h->profile) return;
        if (!h->soloev[g][which] && hipEventCreate(&h->soloev[g][which]) != hipSuccess) { h->soloev[g][which] = nullptr; return; }
        (void)hipEventRecord(h->soloev[g][which], gs[g]);
        if (which == 1 && h->soloev[g][0]) solo_timed[g] = true;
    }

    void queue_window_untimed(int g)            // `check_every` rounds of group g, then the copy of its counters
    {
        GroupRun &r = gr[g];
        const WorkspaceHost &v = gv[g];
        int cur = 0;
        for (int i = 0; i < check_every && r.round < max_rounds; i++) {
            cur = (int)(r.round & 1);
            int *lists = v.lists + (size_t)cur * 2 * v.Ls;
            int *counts = v.counts + cur * 4;
            int *counts_next = v.counts + (cur ^ 1) * 4;
            hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
            // profile mode samples every 8th round: five events per sampled launch set
            if (h->profile && (r.round & 7) == 0 && get_event(h, nev + 4)) { // all five exist, or none is used
                for (int k = 0; k < 5; k++) ev[k] = h->ev_pool[nev + k];
                nev += 5;
            }
            if (ev[0]) (void)hipEventRecord(ev[0], gs[g]);
            launch_step(h, v, gs[g], lists, counts, counts_next, r.slot_bound, cur);
            if (ev[1]) (void)hipEventRecord(ev[1], gs[g]);
            // (counts[2] of the round's buffer: K1c leaves the number of gradient slots there for the next step
            // kernel's thread-per-agent blocks)
            const bool fused = launch_eval(h, v, gs[g], lists, counts, 0, 0, ev[2], ev[3], r.slot_bound, counts + 2);
            if (ev[4]) (void)hipEventRecord(ev[4], gs[g]);
            r.round++;
            rounds_done[g]++;
            launch_sets++;
            unfused_sets += !fused;
        }
        // (an event query that says "not ready" is recorded as the thread's last error too: not a failure)
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess && le != hipErrorNotReady) { rc_loop = MPC_E_HIP; return; }
        const int wb = (int)(r.window & 1);
        if (!h->pollev[wb][g] && hipEventCreateWithFlags(&h->pollev[wb][g], hipEventDisableTiming) != hipSuccess) { rc_loop = MPC_E_HIP; return; }
        if (hipMemcpyAsync(h->pinned().poll[wb][g], v.counts + cur * 4, 2 * sizeof(int), hipMemcpyDeviceToHost, gs[g]) != hipSuccess ||
            hipEventRecord(h->pollev[wb][g], gs[g]) != hipSuccess) { rc_loop = MPC_E_HIP; return; }
        r.window++;
    }
    void queue_window(int g)
    {
        if (!host_timing) { queue_window_untimed(g); return; }
        const auto t0 = std::chrono::steady_clock::now();
        queue_window_untimed(g);
        host_queue_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }

    // what the counters of window `pb` say about group g; returns false when the group is done with rounds
    bool decide(int g, int pb)
    {
        const int *polled = h->pinned().poll[pb][g];
        const int reqs = polled[0] + polled[1];
        if (reqs == 0) return false;
        gr[g].slot_bound = std::min(gr[g].slot_bound, 2 * reqs);
        if (solo_ok && h->solo_max > 0 && reqs <= h->solo_max) {
            // few agents left in this group: they finish in the persistent kernel, each in
            // its own wave, instead of waiting for four launches per evaluation
            hand_to_solo(g, w.solo_ctr + 2 * g, true, reqs);
            return false;
        }
        return true;
    }

    // Every group advances on its own: a window of `check_every` rounds is queued, its request counters are
    // copied back behind it, and the host looks at them ONE WINDOW LATE -- a second window is already queued
    // by then, so the stream does not run dry while the host decides.  The host serves whichever group's
    // counters have arrived (event query, no blocking wait on one group while another's stream empties:
    // the lock-step loop of round 1 left 60 - 200 us bubbles per window on the groups it was not waiting
    // for, ~6 % of their streams' time in the r02d trace).
    void run_rounds()
    {
        if (all_solo) {
            hand_to_solo(0, w.solo_ctr, false, B);
            gr[0].active = false; nactive = 0;
        }
        t_loop0 = std::chrono::steady_clock::now();
        // (tried: the groups started 40 / 80 / 160 us apart, so that one's step kernel meets another's K1 -- no change)
        for (int g = 0; g < ng && nactive > 0; g++) queue_window(g);
        for (int g = 0; g < ng && nactive > 0; g++) if (gr[g].round < max_rounds) queue_window(g);
        // The host has nothing to do while the windows it has queued run (milliseconds with all agents active):
        // it spins on the event queries only for a short while after the last progress, then sleeps in short naps
        // -- a second window is always queued behind the one polled, so a nap delays no launch -- and leaves its
        // core to whoever needs it (eight ranks on one node are eight of these loops: INTEGRATION.md 4).
        // MPC_SPIN=1 keeps the pure busy-wait.
        auto last_progress = std::chrono::steady_clock::now();
        while (nactive > 0 && rc_loop == MPC_OK) {
            bool progressed = false;
            for (int g = 0; g < ng; g++) {
                GroupRun &r = gr[g];
                if (!r.active) continue;
                const long long oldest = r.window - (r.window >= 2 ? 2 : 1);    // the window whose counters are looked at next
                const int pb = (int)(oldest & 1);
                const hipError_t q = hipEventQuery(h->pollev[pb][g]);
                if (q == hipErrorNotReady) continue;
                if (q != hipSuccess) { rc_loop = MPC_E_HIP; break; }
                progressed = true;
                if (host_timing && r.window - oldest > 1 && hipEventQuery(h->pollev[pb ^ 1][g]) == hipSuccess) {
                    // both queued windows have run: this group's stream was empty while the host was elsewhere
                    if (dry_windows++ == 0) first_dry_round = r.round;
                }
                if (host_trace)
                    trace.push_back({(long long)g, r.round - (r.window - oldest) * check_every + check_every - 1,
                                     (long long)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_loop0).count(),
                                     (long long)(h->pinned().poll[pb][g][0] + h->pinned().poll[pb][g][1])});
                bool go = decide(g, pb);
                if (go && r.round >= max_rounds) {
                    // the round limit: nothing more can be queued; the verdict is the LAST window's
                    if (r.window - oldest > 1) {
                        if (hipEventSynchronize(h->pollev[pb ^ 1][g]) != hipSuccess) { rc_loop = MPC_E_HIP; break; }
                        go = decide(g, pb ^ 1);
                    }
                    if (go) { rc_loop = MPC_E_LIMIT; break; }
                }
                if (!go) { r.active = false; nactive--; continue; }
                queue_window(g);
            }
            if (progressed) { last_progress = std::chrono::steady_clock::now(); continue; }
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - last_progress).count() > h->poll_timeout_s) {
                h->timed_out = true; rc_loop = MPC_E_HIP; break;      // no window has completed for poll_timeout_s
            }
            if (h->spin || std::chrono::steady_clock::now() - last_progress < std::chrono::microseconds(40))
                __builtin_ia32_pause();
            else
                std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
    }

    void report_host_timing() const
    {
        if (host_timing)
            fprintf(stderr, "[mpc host] round loop %.2f ms, of which queueing launches %.2f ms (%lld launch sets, %d groups); "
                            "windows found with the stream already empty: %lld (first at round %lld)\n",
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_loop0).count(),
                    host_queue_s * 1e3, launch_sets, ng, dry_windows, first_dry_round);
        if (FILE *f = host_trace ? fopen(h->host_trace.c_str(), "a") : nullptr) {
            fprintf(f, "# solve: group, last round of the window, us since the loop began, requests of that round\n");
            for (const auto &t : trace) fprintf(f, "%lld %lld %lld %lld\n", t[0], t[1], t[2], t[3]);
            fclose(f);
        }
    }

    // how the round loop ended; then the groups' streams join the caller's and the totals of the solve are read
    int join_and_read_totals()
    {
        if (rc_loop == MPC_E_LIMIT) return fail(MPC_E_LIMIT, "mpc_solve_batch: round limit reached");
        if (h->timed_out)
            return fail(MPC_E_HIP, "mpc_solve_batch: wall-clock bound of " + std::to_string(h->poll_timeout_s) +
                                   " s expired in the round loop: no polled window completed (mpc_set_poll_timeout); work is still queued");
        if (rc_loop != MPC_OK) return fail(rc_loop, "mpc_solve_batch: HIP error in the round loop");
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess && le != hipErrorNotReady) return fail(MPC_E_HIP, std::string("mpc_solve_batch: ") + hipGetErrorString(le));
        if (ng > 1) { // join
            for (int g = 0; g < ng; g++) {
                HIPCHK(hipEventRecord(h->gevent[g], gs[g]));
                HIPCHK(hipStreamWaitEvent(s, h->gevent[g], 0));
            }
        }
        for (int g = 0; g < ng; g++) h->rounds = std::max<int64_t>(h->rounds, rounds_done[g]);
        unsigned long long *tot = h->pinned().totals;
        int *sctr = h->pinned().solo_ctr;
        hipLaunchKernelGGL(totals_kernel, grid_for(B, 256), dim3(256), 0, s, w);
        HIPCHK(hipMemcpyAsync(tot, w.totals, sizeof(PinnedCounts::totals), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(sctr, w.solo_ctr, sizeof(PinnedCounts::solo_ctr), hipMemcpyDeviceToHost, s));
        { const int rs = bounded_sync(h, s, "mpc_solve_batch"); if (rs) return rs; }
        h->evals_grad = (int64_t)tot[0]; h->evals_cost = (int64_t)tot[1]; h->lbfgs_rows = (int64_t)tot[2];
        h->spec_issued = (int64_t)tot[4]; h->spec_used = (int64_t)tot[5];
        h->la_evals = (int64_t)tot[7]; h->la_hits = (int64_t)tot[8];
        if (all_solo) h->solo_agents = B;
        else for (int g = 0; g < ng; g++) h->solo_agents += sctr[2 * g + 1];
        // every agent must have reached PH_DONE: the round path says so through its request counters, the
        // persistent kernel only through the records (its trip guard leaves an agent where it stands)
        if (tot[6] != 0)
            return fail(MPC_E_LIMIT, "mpc_solve_batch: round limit reached (" + std::to_string(tot[6]) +
                                     " agents unfinished in the persistent kernel)");
        return MPC_OK;
    }

    // profile mode: the sampled events become the handle's per-kernel milliseconds; always: its launch counts
    int reduce_profile()
    {
        if (h->profile) {
            { const int rs = bounded_sync(h, s, "mpc_solve_batch"); if (rs) return rs; }
            for (size_t i = 0; i + 4 < nev; i += 5) {
                for (int k = 0; k < 4; k++) {
                    float d = 0.f;
                    (void)hipEventElapsedTime(&d, h->ev_pool[i + k], h->ev_pool[i + k + 1]);
                    h->kernel_ms[k] += d;
                }
            }
            // scale the sampled sums to all launch sets of the solve
            const double sampled = (double)(nev / 5);
            const double scale = sampled > 0 ? (double)launch_sets / sampled : 0.0;
            for (int k = 0; k < 4; k++) h->kernel_ms[k] *= scale;
            h->solo_longest_ms = 0.0;
            for (int g = 0; g < MPC_MAX_GROUPS; g++) {
                float d = 0.f;
                if (solo_timed[g]) (void)hipEventElapsedTime(&d, h->soloev[g][0], h->soloev[g][1]);
                h->kernel_ms[4] += d;                       // summed over the groups (their launches overlap in time)
                h->solo_longest_ms = std::max(h->solo_longest_ms, (double)d);
            }
            h->step_ms = h->kernel_ms[0];
            h->eval_ms = h->kernel_ms[1] + h->kernel_ms[2] + h->kernel_ms[3];
        }
        h->launches = (int64_t)launch_sets;
        h->kernel_launches[0] = h->kernel_launches[1] = h->kernel_launches[2] = launch_sets;
        h->kernel_launches[3] = unfused_sets;
        h->kernel_launches[4] = solo_launches;
        HIPCHK(hipGetLastError());
        return MPC_OK;
    }

    int run()
    {
        if (const int rc = begin()) return rc;
        if (const int rc = plan_groups_and_fork()) return rc;
        run_rounds();
        report_host_timing();
        if (const int rc = join_and_read_totals()) return rc;
        return reduce_profile();
    }
};

// the solve proper; x0 / U / lambda are the caller's buffers, used in place
static int run_solver(mpc_handle *h, hipStream_t s)
{
    h->timed_out = false;
    const int rc = SolveRun(h, s).run();
    // On any failure rounds may still be queued on the sub-batch streams (non-blocking streams: a
    // wait on `s` does not cover them) and they write into the caller's U / lambda and the arena:
    // nothing is handed back to the caller before the device has drained -- EXCEPT after the wall-clock
    // bound: the device is not answering, a blocking wait would be the hang the bound exists to end.  The
    // caller gets MPC_E_HIP and must treat the buffers of this solve as in use until it has synchronised the
    // device itself (or given up on it).
    if (rc != MPC_OK && !h->timed_out) {
        const std::string keep = g_err;
        (void)hipDeviceSynchronize();
        g_err = keep;
    }
    return rc;
}
