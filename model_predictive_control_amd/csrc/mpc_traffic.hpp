// mpc_traffic.hpp -- the kernel of mpc_opponents_from_plans and mpc_closed_loop_traffic: for every agent the NDISC nearest
// agents of its scene, by the smallest value the disc constraint takes along everybody's current plans.  The solver
// kernels are not touched: the traffic loop is mpc_rollout, this selection, mpc_discs_from_plans, the solve and
// plant_step_kernel, launched one after the other.
#pragma once
#include "mpc_event.hpp"

namespace mpc {

constexpr int SCENE_MAX = 64;      // agents per scene at most (MPC_SCENE_MAX): one lane per opponent
constexpr int TR_BLK = 256;        // threads per workgroup (four waves)
constexpr int TR_KC = 32;          // stages of the workgroup's agents held in LDS at a time: 2 x 32 x 64 doubles = 32 KB

// g = (dx dx + dy dy) - r2 with every operation rounded on its own: K1b's disc expression (stage_record) and
// tests/discs_common.disc_g, operand for operand (r2 = r r, rounded once by the caller)
MPC_DEV double traffic_g(double bx, double by, double ox, double oy, double r2)
{
#pragma clang fp contract(off)
    const double dx = bx - ox, dy = by - oy;
    return (dx * dx + dy * dy) - r2;
}
MPC_DEV double traffic_sq(double r)
{
#pragma clang fp contract(off)
    return r * r;
}

// Scenes are blocks of G consecutive agents (B % G == 0).  A workgroup takes SPW = max(1, 64 / Gp) whole scenes (Gp: G
// rounded up to a power of two), at most 64 agents, and stages their (x, y) of TR_KC stages in LDS: every position is
// read G times from there.  Plans of more than TR_KC stages are staged chunk by chunk once per pass of the workgroup over
// its agents (up to 16 passes at G = 64), i.e. read that often from global memory: the horizons in use (N <= 32) take
// one chunk, staged once.  A wave holds 64 / Gp agents at a time, Gp lanes each, lane `ol` of an agent looking at opponent `ol` of
// the agent's scene; c = min_k g_k over the stages (a non-finite g_k takes the pair out), then NDISC rounds of an
// arg-min butterfly on (c, ol) inside the agent's Gp lanes (xor offsets below Gp never leave them).  No atomics; a
// min of doubles does not depend on the order, so chunking the stages changes no bit.
// Outputs, each optional: opp [B][NDISC] global indices (-1: none); opp_rec, the same words at opp_rec[b * rec_stride + j];
// clear at clear[b * clear_stride + j] for j < clear_slots (+inf: none).
// HELD (mpc_opponent_trigger; hd = held [B]): the lane's own agent b folds its first n_b = held_stages(held[b], Nst) stages
// alone -- the stages a plan of Nst of which held[b] have been applied still holds, as mpc_rollout_held lays them out.  The
// count is the agent's, not the opponent's: opponent o is read at the stages j < n_b as X has them, its own repeated tail
// included (what o goes on applying as far as anyone knows, and what a gather at this step copies).  Every stage is staged
// like before (X has Nst stages); the tail behind n_b is never compared, so a non-finite g_j there does not take the pair
// out.  Everything else is the same code.
MPC_DEV int held_stages(int held, int N) { return N - max(0, min(held, N - 1)); }
template <bool HELD = false, class... HD>
__global__ void __launch_bounds__(TR_BLK) opponents_kernel(int B, int G, int Gp, int spw, int Nst, int nx,
                                                           const double *__restrict__ X, const double *__restrict__ radius,
                                                           double reach2, int *__restrict__ opp, int *__restrict__ opp_rec,
                                                           size_t rec_stride, double *__restrict__ clear, size_t clear_stride,
                                                           int clear_slots, HD... hd)
{
    static_assert(sizeof...(HD) == (HELD ? 1 : 0), "the held form takes held [B], the plain form nothing");
    __shared__ double s_x[TR_KC * SCENE_MAX], s_y[TR_KC * SCENE_MAX];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t b0 = (size_t)blockIdx.x * spw * G;                 // first agent of the workgroup (a scene's first)
    const int A = (int)min((size_t)spw * G, (size_t)B - b0);         // its agents: whole scenes, 1 .. 64
    const int apw = 64 / Gp;                                         // agents per wave and pass
    const int passes = (A + (TR_BLK / 64) * apw - 1) / ((TR_BLK / 64) * apw);
    const int nch = (Nst + TR_KC - 1) / TR_KC;
    const int ol = lane & (Gp - 1);
    const double inf = __builtin_inf();
    for (int pass = 0; pass < passes; pass++) {
        const int a = (pass * (TR_BLK / 64) + wv) * apw + lane / Gp;  // the lane's agent within the workgroup
        const bool agent_on = a < A;
        const int sc0 = agent_on ? (a / G) * G : 0;                  // first agent of its scene within the workgroup
        const int o = sc0 + ol;                                      // the lane's opponent within the workgroup
        const bool pair_on = agent_on && ol < G && o != a;
        const int ar = agent_on ? a : 0, orr = pair_on ? o : 0;      // what the lane reads (in range whatever it is)
        const double r2 = pair_on ? traffic_sq(radius[b0 + orr]) : 0.0;
        double c = inf;
        bool bad = false;
        int nb = Nst;                                                // the stages the lane's agent compares
        if constexpr (HELD) {
            const int *__restrict__ held = (hd, ...);
            nb = agent_on ? held_stages(held[b0 + a], Nst) : 0;
        }
        for (int ch = 0; ch < nch; ch++) {
            const int k0 = ch * TR_KC, kc = min(TR_KC, Nst - k0);
            if (nch > 1 || pass == 0) {                              // (uniform over the workgroup)
                __syncthreads();                                     // the chunk before has been read by everyone
                for (int i = threadIdx.x; i < A * kc; i += TR_BLK) {       // the agent runs fastest: consecutive LDS words
                    const int k = i / A, ai = i - k * A;
                    const double *__restrict__ p = X + ((b0 + ai) * (size_t)Nst + (size_t)(k0 + k)) * nx;
                    s_x[k * SCENE_MAX + ai] = p[0];
                    s_y[k * SCENE_MAX + ai] = p[1];
                }
                __syncthreads();
            }
            int kend = kc;
            if constexpr (HELD) kend = min(kc, nb - k0);             // (<= 0 behind the agent's last stage)
            for (int k = 0; k < kend; k++) {
                const double g = traffic_g(s_x[k * SCENE_MAX + ar], s_y[k * SCENE_MAX + ar], s_x[k * SCENE_MAX + orr],
                                           s_y[k * SCENE_MAX + orr], r2);
                if (!isfinite(g)) bad = true;
                else if (g < c) c = g;
            }
        }
        const int none = 0x7fffffff;
        const bool cand = pair_on && !bad && c < reach2;
        double kc_ = cand ? c : inf;                                 // the lane's key (c, ol); (+inf, none): no candidate
        int ki = cand ? ol : none;
        for (int j = 0; j < NDISC; j++) {
            double bc = kc_;
            int bi = ki;
            for (int off = Gp >> 1; off; off >>= 1) {
                const double oc = __shfl_xor(bc, off);
                const int oi = __shfl_xor(bi, off);
                if (oc < bc || (oc == bc && oi < bi)) { bc = oc; bi = oi; }
            }
            // every lane of the agent holds the winner; a candidate's c is finite, so bi == none iff nobody is left
            if (agent_on && ol == 0) {
                const size_t b = b0 + a;
                const int og = bi == none ? -1 : (int)(b0 + sc0 + bi);
                if (opp) opp[b * NDISC + j] = og;
                if (opp_rec) opp_rec[b * rec_stride + j] = og;
                if (clear && j < clear_slots) clear[b * clear_stride + j] = bi == none ? inf : bc;
            }
            if (ki == bi) { kc_ = inf; ki = none; }                  // the winner leaves the next round
        }
    }
}

} // namespace mpc
