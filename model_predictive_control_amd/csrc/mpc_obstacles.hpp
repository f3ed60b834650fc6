// mpc_obstacles.hpp -- the kernels of mpc_obstacles_select, mpc_discs_from_obstacles / mpc_fields_from_obstacles and
// mpc_closed_loop_obstacles: scripted moving obstacles.  Every scene (a block of G consecutive agents) has K obstacle
// tracks of Lt samples, one per Ts, shared by its agents: obs [B / G][K][Lt][W], W = 3 (cx, cy, r) on a handle of
// MPC_CONSTR_DISCS and W = NFSRC (a whole risk source) on every other.  The selection is opponents_kernel's rule with the
// opponents' plans replaced by the time-shifted window of the tracks; the gather writes the window of the selected
// tracks into the bound table.  The solver kernels and opponents_kernel are not touched.
#pragma once
#include "mpc_traffic.hpp"

namespace mpc {

constexpr int OB_KC = 16;          // stages of the workgroup's windows and plans held in LDS at a time
constexpr int OB_LD = SCENE_MAX + 1;   // LDS words per stage: one more than the 64 columns, so that staging (the stage runs
                                       // fastest, as in global memory) does not hit one bank with every lane
constexpr int OB_PASSES = SCENE_MAX / (TR_BLK / 64);   // passes of a workgroup over its agents at most (Kp = 64: 4 agents a pass)
static_assert(OB_KC * OB_LD * 5 * sizeof(double) <= 64 * 1024, "obstacles_kernel: static LDS of a workgroup");

// the sample of time i >= 0 of a track of Lt samples, in integers: periodic, or standing at the last sample
MPC_DEV int obstacle_sample(int i, int Lt, int wrap) { return wrap ? i % Lt : min(i, Lt - 1); }
// word of a sample that says "absent" when it is zero: r of a disc, A of a source
template <int W> MPC_DEV constexpr int obstacle_key() { return W == 3 ? 2 : 4; }

// A workgroup takes SPW = max(1, 64 / max(Gp, Kp)) whole scenes (Gp, Kp: G, K rounded up to a power of two): at most 64
// agents and 64 tracks.  Per chunk of OB_KC stages it stages, each word read from global memory once, the window of every
// track as (cx, cy, r2) -- r2 = r r for discs, 0 for fields, -1 for an absent sample -- and the (x, y) of every agent,
// then every lane folds the chunk into its min.  A wave holds 64 / Kp agents at a time, Kp lanes each, lane `ol` of an
// agent looking at track `ol` of the agent's scene; the workgroup passes over its agents (up to OB_PASSES times, the
// running minima in registers), and at the end NDISC rounds of opponents_kernel's arg-min butterfly on (c, ol) run inside
// the agent's Kp lanes.  No atomics; a min of doubles does not depend on the order, so chunking changes no bit.
// Outputs as in opponents_kernel, sel holding the track's index WITHIN the scene: sel [B][NDISC] (-1: none); sel_rec, the
// same words at sel_rec[b * rec_stride + j]; clear at clear[b * clear_stride + j] for j < clear_slots (+inf: none).
// HELD (mpc_obstacle_trigger; hd = held [B]): agent b folds its first held_stages(held[b], Nst) (mpc_traffic.hpp) stages alone -- the stages
// a plan of Nst of which held[b] have been applied still holds, as mpc_rollout_held lays them out; the tail that repeats
// the last input is staged like every stage (X has Nst stages) and never compared.  Everything else is the same code.
// (The count is re-read from held per chunk and pass; 16 counts kept in registers cost 64 vector registers.)
template <int W, bool HELD = false, class... HD>
__global__ void __launch_bounds__(TR_BLK) obstacles_kernel(int B, int G, int K, int Kp, int spw, int Lt, int wrap, int ti, int Nst,
                                                           int nx, const double *__restrict__ X, const double *__restrict__ obs,
                                                           double reach2, int *__restrict__ sel, int *__restrict__ sel_rec,
                                                           size_t rec_stride, double *__restrict__ clear, size_t clear_stride,
                                                           int clear_slots, HD... hd)
{
    static_assert(sizeof...(HD) == (HELD ? 1 : 0), "the held form takes held [B], the plain form nothing");
    __shared__ double s_ox[OB_KC * OB_LD], s_oy[OB_KC * OB_LD], s_r2[OB_KC * OB_LD], s_x[OB_KC * OB_LD], s_y[OB_KC * OB_LD];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t b0 = (size_t)blockIdx.x * spw * G;                 // first agent of the workgroup (a scene's first)
    const size_t sc0 = (size_t)blockIdx.x * spw;                    // its first scene
    const int A = (int)min((size_t)spw * G, (size_t)B - b0);         // its agents: whole scenes, 1 .. 64
    const int nob = (A / G) * K;                                     // its tracks, 1 .. 64
    const int apw = 64 / Kp;                                         // agents per wave and pass
    const int passes = (A + (TR_BLK / 64) * apw - 1) / ((TR_BLK / 64) * apw);
    const int ol = lane & (Kp - 1);
    const double inf = __builtin_inf();
    double c[OB_PASSES];
    unsigned bad = 0;                                                // bit `pass`: a g_k of the pair was not finite
#pragma unroll
    for (int pass = 0; pass < OB_PASSES; pass++) c[pass] = inf;
    for (int k0 = 0; k0 < Nst; k0 += OB_KC) {
        const int kc = min(OB_KC, Nst - k0);
        if (k0) __syncthreads();                                     // the chunk before has been read by everyone
        for (int i = threadIdx.x; i < nob * kc; i += TR_BLK) {       // the stage runs fastest: consecutive samples of a track
            const int oi = i / kc, k = i - oi * kc;
            const double *__restrict__ p = obs + (((sc0 + oi / K) * K + oi % K) * (size_t)Lt +
                                                  (size_t)obstacle_sample(ti + k0 + k, Lt, wrap)) * W;
            const double key = p[obstacle_key<W>()];
            s_ox[k * OB_LD + oi] = p[0];
            s_oy[k * OB_LD + oi] = p[1];
            s_r2[k * OB_LD + oi] = key == 0.0 ? -1.0 : W == 3 ? traffic_sq(key) : 0.0;
        }
        for (int i = threadIdx.x; i < A * kc; i += TR_BLK) {
            const int ai = i / kc, k = i - ai * kc;
            const double *__restrict__ p = X + ((b0 + ai) * (size_t)Nst + (size_t)(k0 + k)) * nx;
            s_x[k * OB_LD + ai] = p[0];
            s_y[k * OB_LD + ai] = p[1];
        }
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < OB_PASSES; pass++) {
            if (pass < passes) {                                     // (uniform over the workgroup)
                const int a = (pass * (TR_BLK / 64) + wv) * apw + lane / Kp;   // the lane's agent within the workgroup
                const bool pair_on = a < A && ol < K;
                const int ar = pair_on ? a : 0, orr = pair_on ? (a / G) * K + ol : 0;   // what the lane reads (in range whatever it is)
                double cm = c[pass];
                bool bd = false;
                int kend = kc;
                if constexpr (HELD) {                                // the stages the lane's agent still compares (a cached
                    const int *__restrict__ held = (hd, ...);        // load per chunk: no count is kept in registers)
                    kend = min(kc, (a < A ? held_stages(held[b0 + a], Nst) : 0) - k0);   // (<= 0 behind its last stage)
                }
                for (int k = 0; k < kend; k++) {
                    const double r2 = s_r2[k * OB_LD + orr];
                    if (r2 < 0.0) continue;                          // absent at this stage (a NaN radius is present, and takes the pair out)
                    const double g = traffic_g(s_x[k * OB_LD + ar], s_y[k * OB_LD + ar], s_ox[k * OB_LD + orr], s_oy[k * OB_LD + orr], r2);
                    if (!isfinite(g)) bd = true;
                    else if (g < cm) cm = g;
                }
                c[pass] = cm;
                if (bd) bad |= 1u << pass;
            }
        }
    }
    const int none = 0x7fffffff;
#pragma unroll
    for (int pass = 0; pass < OB_PASSES; pass++) {
        if (pass < passes) {
            const int a = (pass * (TR_BLK / 64) + wv) * apw + lane / Kp;
            const bool agent_on = a < A;
            // a track with no present sample in the window kept c = +inf: no candidate, whatever reach is
            const bool cand = agent_on && ol < K && !(bad >> pass & 1u) && c[pass] < reach2;
            double kc_ = cand ? c[pass] : inf;                       // the lane's key (c, ol); (+inf, none): no candidate
            int ki = cand ? ol : none;
            for (int j = 0; j < NDISC; j++) {
                double bc = kc_;
                int bi = ki;
                for (int off = Kp >> 1; off; off >>= 1) {
                    const double oc = __shfl_xor(bc, off);
                    const int oi = __shfl_xor(bi, off);
                    if (oc < bc || (oc == bc && oi < bi)) { bc = oc; bi = oi; }
                }
                // every lane of the agent holds the winner; a candidate's c is finite, so bi == none iff nobody is left
                if (agent_on && ol == 0) {
                    const size_t b = b0 + a;
                    const int og = bi == none ? -1 : bi;
                    if (sel) sel[b * NDISC + j] = og;
                    if (sel_rec) sel_rec[b * rec_stride + j] = og;
                    if (clear && j < clear_slots) clear[b * clear_stride + j] = bi == none ? inf : bc;
                }
                if (ki == bi) { kc_ = inf; ki = none; }              // the winner leaves the next round
            }
        }
    }
}

// mpc_discs_from_obstacles (W = 3) and mpc_fields_from_obstacles (W = NFSRC): table[b][k][j] = the W words of sample
// (ti + k) of track sel[b][j] of agent b's scene; W zeros where sel[b][j] is outside [0, K) and where the sample is
// absent (its other words are not read).  One thread per (agent, stage, slot); every word written is a copy of an input
// word or zero.
// MASKED (step 7 of mpc_closed_loop_obstacles_event; mk = (mask [B], sel_plan [B][NDISC])): the rows of the agents with
// mask[b] != 0 alone are written -- a held agent's row stays the one its plan was solved on -- and for those agents
// sel_plan[b] <- sel[b] (the thread of stage 0 writes it): the tracks the plan about to be solved is solved against.
// (RowMask: mpc_event.hpp, beside the masked gathers from plans)
template <int W, bool MASKED = false, class... MK>
__global__ void __launch_bounds__(256) rows_from_obstacles_kernel(int B, int N, int G, int K, int Lt, int wrap, int ti,
                                                                  const double *__restrict__ obs, const int *__restrict__ sel,
                                                                  double *__restrict__ table, MK... mk)
{
    static_assert(NDISC == NFIELD, "one sel [B][2] serves the disc and the field table");
    static_assert(sizeof...(MK) == (MASKED ? 1 : 0), "the masked form takes a RowMask, the plain form nothing");
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)B * N * NDISC) return;
    const int j = (int)(t % NDISC);
    const size_t bk = t / NDISC;
    const int k = (int)(bk % N), b = (int)(bk / N);
    const int o = sel[(size_t)b * NDISC + j];
    if constexpr (MASKED) {
        const RowMask m = (mk, ...);
        if (m.mask[b] == 0) return;
        if (k == 0) m.sel_plan[(size_t)b * NDISC + j] = o;
    }
    double *out = table + t * W;
    const double *__restrict__ p = nullptr;
    if (o >= 0 && o < K) {
        p = obs + (((size_t)(b / G) * K + o) * (size_t)Lt + (size_t)obstacle_sample(ti + k, Lt, wrap)) * W;
        if (p[obstacle_key<W>()] == 0.0) p = nullptr;
    }
#pragma unroll
    for (int i = 0; i < W; i++) out[i] = p ? p[i] : 0.0;
}

// The obstacle rule of mpc_obstacle_trigger on the held-window selection (sel_chk, clear_chk [B][NDISC]; one thread per
// agent): why[b] bit 0 = fire_in[b] != 0 (null: 0); for held[b] > 0, bit 1 = watch & 1 and !(clear_chk[b][0] >= clear_thr)
// -- +inf, nothing in reach, never fires --, bit 2 = watch & 2 and some sel_chk[b][j] >= 0 is not a member of the SET
// sel_plan[b] (a change of order is no new obstacle).  fire_out[b] = why[b] != 0; why at why[b * why_stride] (null ok).
__global__ void __launch_bounds__(64) obstacle_rule_kernel(int B, const int *__restrict__ held, const int *__restrict__ sel_chk,
                                                           const double *__restrict__ clear_chk, const int *__restrict__ sel_plan,
                                                           double clear_thr, int watch, const int *fire_in,
                                                           int *fire_out, uint8_t *__restrict__ why, size_t why_stride)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int w = fire_in && fire_in[b] != 0 ? 1 : 0;
    if (held[b] > 0) {
        if ((watch & 1) && !(clear_chk[(size_t)b * NDISC] >= clear_thr)) w |= 2;
        if (watch & 2) {
#pragma unroll
            for (int j = 0; j < NDISC; j++) {
                const int o = sel_chk[(size_t)b * NDISC + j];
                bool known = o < 0;
#pragma unroll
                for (int i = 0; i < NDISC; i++) known = known || sel_plan[(size_t)b * NDISC + i] == o;
                if (!known) w |= 4;
            }
        }
    }
    fire_out[b] = w != 0;
    if (why) why[(size_t)b * why_stride] = (uint8_t)w;
}

// mpc_roads_from_script: table[b][k] = the NROAD words of sample (ti + k) of script row sidx[b] -- clamped to the last
// sample or wrapped, the time rule of the obstacles.  One thread per (agent, stage); a plain copy.  (The range of
// sidx is the caller's to check, as every table's row index is; the Python front end does.)
__global__ void __launch_bounds__(256) roads_from_script_kernel(int B, int N, int Lt, int wrap, int ti, const double *__restrict__ script,
                                                                const int *__restrict__ sidx, double *__restrict__ table)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)B * N) return;
    const int k = (int)(t % N), b = (int)(t / N);
    const double *__restrict__ p = script + ((size_t)sidx[b] * (size_t)Lt + (size_t)obstacle_sample(ti + k, Lt, wrap)) * NROAD;
    double *out = table + t * NROAD;
#pragma unroll
    for (int i = 0; i < NROAD; i++) out[i] = p[i];
}

} // namespace mpc
