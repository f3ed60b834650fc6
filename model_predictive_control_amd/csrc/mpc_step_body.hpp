// mpc_step_body.hpp -- the body of the step kernels (mpc_solver.hpp), included once into each of them: step_kernel
// (MPC_STEP_BA false: the handle's box), step_kernel_box (MPC_STEP_BA true: every agent's own box from the bounds table
// MPC_STEP_BT, that kernel's third parameter) and the constraint forms of the two (MPC_STEP_CA, below).  Text, not a function: the kernels re-read their DevCfg and Workspace from
// the argument segment (KernArgs) and step_kernel's instruction stream is pinned -- a body reached through a call, even an
// inlined one, is scheduled differently.  No include guard.
// MPC_STEP_CA true (step_kernel_con, step_kernel_box_con): every agent's own constraint bounds from the constraint table,
// the parameter behind the ones above (KernCon).
//
// The box form: the workgroup's row indices arrive with its phase words (one coalesced read, lane l: agent base + l), so
// an agent's row is addressed from a register, and its two values per lane are asked for with the record and the rows
// of the wave's NEXT agent -- in flight one agent ahead like everything else, never a dependent load where the
// projection needs them.
    // blocks [0, nstep): the wave-per-agent state machine; blocks beyond (c.chain): PH_W_LS_G by one thread per
    // agent for the gradient slots of the round just finished, whose count K1c left in counts_next[2] (the buffer
    // of that round: this kernel zeroes its two list counters for the round after this one, not that word)
    if ((int)blockIdx.x >= nstep) {
        extern __shared__ double s_chain[];
        if (NE == 1) chain_block<MPC_STEP_BA>(c, w, MPC_STEP_BT, (int)blockIdx.x - nstep, counts_next[2], par, lists_out, counts_out, s_chain);
        return;
    }
    // apb = agents per workgroup (64, 16 or 4): a wave walks its agents one after the other, so a small
    // batch is spread over more workgroups (one agent per wave at apb = 4) -- latency, not throughput
    __shared__ int s_req[64];
    __shared__ int s_next;
    extern __shared__ double s_hist[];                   // MC < 0: 2 M n doubles per wave
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#if MPC_DEV_STAMP == 3
    DevStamp stamp(blockIdx.x * STEP_WAVES + wv);
#endif
    double *hist = s_hist + (MC < 0 ? (size_t)wv * 2 * P * c.n : 0);
    if (blockIdx.x == 0 && threadIdx.x == 0) { counts_next[0] = 0; counts_next[1] = 0; } // next round's buffer
    // Which of the workgroup's agents are still running: one coalesced look at their phase words.
    // Only the running ones are handed to the waves, so a wave never pays a memory round trip to
    // find out that an agent is finished.
    const int base = blockIdx.x * apb;
    const int phw = lane < apb && base + lane < w.B ? rec_int_of(w.rec[(size_t)(base + lane) * REC + R_PHASE]) : 0;
    int brow = 0;                                        // (BA) row of the bounds table of agent base + lane
    if constexpr (MPC_STEP_BA) brow = lane < apb && base + lane < w.B ? (MPC_STEP_BT).bidx[base + lane] : 0;
    using CON = ConOf<MPC_STEP_CA, KernCon<MPC_STEP_BA>>;
    using BOX = BoxOf<MPC_STEP_BA, LaneBox>;
    const auto box_of = [&](const BoxTab &b, int l) {
        if constexpr (MPC_STEP_BA) return load_lane_box(b, __builtin_amdgcn_readlane(brow, l), lane);
        else return CfgBox();
    };
    // (PH_DONE == 0; with c.chain an agent that waits in PH_W_LS_G is served by a chain_block of this launch)
    const bool runnable = phw != 0 && !(c.chain && (phw == PH_W_LS_G || phw == PH_W_LS_C + chain_tag(par)));
    const unsigned long long act = __ballot(runnable);
    const int rank = __popcll(act & ((1ull << lane) - 1ull));
    const int nact = __popcll(act);
    if (threadIdx.x == 0) s_next = 0;
    if (wv == 0) s_req[lane] = REQ_NONE;
    __syncthreads();
    // the waves take the running agents from a shared counter, one ahead of the one they work on (its
    // rows are in flight meanwhile): an agent-step costs between ~0.3 and ~3 us depending on its phase,
    // and a static deal leaves three waves waiting for the unlucky one
    auto claim = [&]() -> int {
        int i = 0;
        if (lane == 0) i = atomicAdd(&s_next, 1);
        i = __builtin_amdgcn_readfirstlane(i);
        if (i >= nact) return -1;
        return (int)__builtin_ctzll(__ballot(runnable && rank == i));
    };
    AgentIn<NE> nxt;
    BOX nbx{};
    int loc = claim();
    // (MPC_ALL_ROWS: the six-row fetch of rounds 1 - 2, for the A/B measurement and the bit-identity test)
    const auto phase_of = [&](const DevCfg &cc, int l) { return cc.all_rows ? -1 : (__builtin_amdgcn_readlane(phw, l) & PH_MASK); };
    if (loc >= 0) { nxt = load_agent<NE>(c, w, base + loc, lane, phase_of(c, loc)); nbx = box_of(MPC_STEP_BT, loc); }
    while (loc >= 0) {
        // (the kernel's parameters c and w are not used inside this loop: see KernArgs)
        const KernArgs ka;
        const DevCfg &c = ka.c();
        const Workspace &w = ka.w();
        const int a = base + loc;
        const AgentIn<NE> cur = nxt;
        const BOX cbx = nbx;
        const int loc_next = claim();
        if (loc_next >= 0) {                             // in flight during agent a
            nxt = load_agent<NE>(c, w, base + loc_next, lane, phase_of(c, loc_next));
            if constexpr (MPC_STEP_BA) nbx = box_of(ka.box(), loc_next);
        }
        bool hist_ready = false;
        if (MC < 0) {
            // An agent that comes back from its Hessian-vector evaluation (or from the cost of a trial
            // whose speculative gradient is there) runs the two-loop almost first thing: start the
            // LDS-DMA of its history now.  Issued BEHIND the next agent's row loads: the wait for the
            // history drains the wave's vector-memory queue in order, so nothing younger than what it
            // needs should be in it.
            const int rlo = __double2loint(cur.rv);      // (the integers of the record: rec_int)
            const int ph = __builtin_amdgcn_readlane(rlo, R_PHASE) & PH_MASK;
            const int hi = __builtin_amdgcn_readlane(rlo, R_LIDX), hf = __builtin_amdgcn_readlane(rlo, R_LFULL);
            const int hl = hi | hf;
            const int sp = __builtin_amdgcn_readlane(rlo, R_SPEC);
            if ((ph == PH_W_HESS || (ph == PH_W_LS_C && sp != 0)) && hl != 0) {
                hist_dma(w.S + (size_t)a * c.M * c.n, w.Y + (size_t)a * c.M * c.n, hist, P * c.n,
                         (hf ? c.M : hi) * c.n, lane);
                hist_ready = true;
            }
        }
#if MPC_DEV_STAMP == 3
        stamp.nfall++;                                   // agent-steps of this wave
        const long long tv0 = __builtin_amdgcn_s_memrealtime();
        const int ph_in = __builtin_amdgcn_readlane(__double2loint(cur.rv), R_PHASE) & PH_MASK;
#endif
        const int req = advance_agent<NE, MC, HASM, true, BOX, CON>(c, w, a, lane, cur, hist, hist_ready, true, /*allow_chain=*/true, P, cbx, CON());
#if MPC_DEV_STAMP == 3
        {   // the longest agent-step of this wave: its length in 10 ns ticks (nmid, capped at 255) and the phase it came in with (nslow)
            const int dt = (int)(__builtin_amdgcn_s_memrealtime() - tv0);
            if (dt > stamp.nmid) { stamp.nmid = dt > 255 ? 255 : dt; stamp.nslow = ph_in; }
        }
#endif
        if (lane == 0) s_req[loc] = req;
        loc = loc_next;
    }
    __syncthreads();
    // (CA: the two list pointers are read again from the argument segment here, where they are used, and so are not held
    // across the loop above -- four scalar registers that the constrained kernels, at 106 of 106, do not have)
    int *lists_o = lists_out, *counts_o = counts_out;
    if constexpr (MPC_STEP_CA) {
        const KernArgs kt;
        lists_o = kt.con_tail(MPC_STEP_BA, 0); counts_o = kt.con_tail(MPC_STEP_BA, 1);
    }
    if (wv == 0) {
        const int r = s_req[lane];
#pragma unroll
        for (int kind = 0; kind < 2; kind++) { // 0: gradient list (normal or channel 2), 1: cost list
            const bool on = kind == 0 ? (r & (REQ_GRAD | REQ_SPEC)) != 0 : (r & REQ_COST) != 0;
            const unsigned long long bal = __ballot(on);
            const int cnt = __popcll(bal);
            if (cnt == 0) continue;                      // uniform
            int base = 0;
            if (lane == 0) base = atomicAdd(&counts_o[kind], cnt);
            base = __builtin_amdgcn_readfirstlane(base);
            if (on) {
                const int off = __popcll(bal & ((1ull << lane) - 1ull));
                const int flag = kind == 0 ? ((r & REQ_SPEC) ? CH2_BIT : 0) | ((r & REQ_CHAIN) ? CHAIN_BIT : 0) : 0;
                lists_o[(size_t)kind * w.Ls + base + off] = (blockIdx.x * apb + lane) | flag;
            }
        }
    }
