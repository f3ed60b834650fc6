// mpc_track.hpp -- kernels of lap driving (mpc_track_windows, mpc_track_locate, mpc_track_select,
// mpc_closed_loop_track): a track [K][2L] becomes a table of overlapping windows, each an ordinary centerline row
// [2S], and every agent's row is re-selected on the device whenever it re-plans.  The solver kernels are not touched:
// K1b, the grid of index ranges and the masked solve see a centerline table and a row index, as they always did.
//
// The rule (integers only; the one floating-point decision is the nearest index):
//   window r of track k is row k*R + r and holds track points r*w + i, i < S (mod L on a closed track);
//   an agent on row k*R + r whose nearest index on that row is i stands at track point r*w + i;
//   open:    p = r*w + i - lead,            r' = min(max(floor(p / w), 0), R - 1)      (floor towards minus infinity)
//   closed:  p = (r*w + i - lead) mod L,    r' = p / w                                (0 <= p < L)
// so that, where nothing is clamped, the agent's nearest index on the new row lies in [lead, lead + w).
#pragma once
#include "mpc_event.hpp"

namespace mpc {

struct TrackGeom { int K, L, w, lead, closed, R; };

// the window of track point `along` (64 bits: r*w + i may pass 2^31 on a track close to the int32 limit)
MPC_DEV int track_row(const TrackGeom &g, long long along)
{
    long long p = along - g.lead;
    if (g.closed) {
        p %= g.L;
        if (p < 0) p += g.L;
        return (int)(p / g.w);
    }
    const long long q = p >= 0 ? p / g.w : -((-p + g.w - 1) / g.w);
    return (int)min(max(q, 0ll), (long long)g.R - 1);
}

// mpc_track_windows: a pure gather, one thread per word of `win` (grid-stride: the table may hold more than 2^31
// words).  Reads stay inside the track row: (r*w + i) mod L on a closed track, <= (R-1) w + S - 1 <= L - 1 on an open one.
__global__ void __launch_bounds__(256) track_windows_kernel(const TrackGeom g, int S, const double *__restrict__ track,
                                                            double *__restrict__ win)
{
    const size_t rows = (size_t)g.K * (size_t)g.R, words = rows * 2 * (size_t)S;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < words; t += (size_t)gridDim.x * 256) {
        const size_t row = t / (2 * (size_t)S);
        const int j = (int)(t - row * 2 * (size_t)S), xy = j >= S ? 1 : 0, i = j - xy * S;
        const size_t k = row / (size_t)g.R;
        const long long r = (long long)(row - k * (size_t)g.R);
        long long p = r * g.w + i;
        if (g.closed) p %= g.L;
        win[t] = track[k * 2 * (size_t)g.L + (size_t)xy * (size_t)g.L + (size_t)p];
    }
}

// mpc_track_select, and the step of mpc_closed_loop_track between the trigger and the masked solve (traj_row != null:
// the row in force at step t of every agent, selected or not).  One thread per agent and no early return: the grid
// search's loop is wave-uniform (see errors_kernel); lanes past the batch redo agent 0.  The nearest index comes from
// nearest_lookup on the agent's current row with the tables K1b will use for it: the same index, bit for bit.  An agent
// that is masked out, whose pose is not finite or whose row is not a row of the table is not written.
__global__ void __launch_bounds__(64) track_select_kernel(const DevCfg c, const TrackGeom g, int B, int nx,
                                                          const double *__restrict__ x, const double *__restrict__ win,
                                                          const int *__restrict__ active, const NearTab nt,
                                                          int *__restrict__ cl_index, int *__restrict__ pos,
                                                          int *__restrict__ traj_row, int t, int T)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = a < B;
    const int aa = live ? a : 0;
    const int row = cl_index[aa];
    const int rr = min(max(row, 0), g.K * g.R - 1);            // (the read stays inside the table whatever the caller wrote)
    const double *clp = win + (size_t)rr * 2 * (size_t)c.S;
    const double px = x[(size_t)aa * nx], py = x[(size_t)aa * nx + 1];
    const int idx = nearest_lookup(c, clp, nt, rr, px, py);
    const bool on = live && row == rr && (!active || active[aa] != 0) && isfinite(px) && isfinite(py);
    int nrow = row;
    if (on) {
        const int k = rr / g.R, r = rr - k * g.R;
        const long long along = (long long)r * g.w + idx;
        nrow = k * g.R + track_row(g, along);
        cl_index[a] = nrow;
        if (pos) pos[a] = (int)(g.closed ? along % g.L : along);
    }
    if (live && traj_row) traj_row[(size_t)a * T + t] = nrow;
}

// mpc_track_locate: the first placement.  cL is the handle's configuration with S = L: nearest_index then scans the
// agent's whole track row (candidates 0 .. L-2, first minimum, the one dist2 expression) and the rule above gives the row.
__global__ void __launch_bounds__(64) track_locate_kernel(const DevCfg cL, const TrackGeom g, int B, int nx,
                                                          const double *__restrict__ x, const double *__restrict__ track,
                                                          const int *__restrict__ track_index, int *__restrict__ cl_index)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= B) return;
    const int k = track_index ? track_index[a] : 0;
    if (k < 0 || k >= g.K) return;                             // not a track of the table: not written
    const int ai = nearest_index(cL, track + (size_t)k * 2 * (size_t)g.L, x[(size_t)a * nx], x[(size_t)a * nx + 1]);
    cl_index[a] = k * g.R + track_row(g, ai);
}

} // namespace mpc
