// The program of tests/test_handle_layout_cpu.py: walks every layout of csrc/mpc_arena.hpp on host memory.  For each case
// it measures, mallocs exactly the measured size, places, writes every block through its placed pointer to its full
// extent (the extents are written out here, from the shapes the structs document -- not taken from the layout) and prints
//   arena <name> <measured bytes>
//   blk <name> <offset> <bytes> <element size>
// for the test to check.  Built for the host alone with the address and undefined-behaviour sanitizers; makes no HIP call.
#include "../model_predictive_control_amd/csrc/mpc_arena.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

struct Arena {
    char *base;
    size_t bytes;
    template <class Layout> Arena(const char *name, Layout layout)
    {
        Carver measure;
        layout(measure);
        bytes = measure.off;
        base = (char *)malloc(bytes);
        if (!base) { fprintf(stderr, "malloc(%zu) failed\n", bytes); exit(2); }
        Carver place(base);
        layout(place);
        if (place.off != bytes) { fprintf(stderr, "%s: placed %zu bytes, measured %zu\n", name, place.off, bytes); exit(3); }
        printf("arena %s %zu\n", name, bytes);
    }
    ~Arena() { free(base); }
    template <class T> void blk(const char *name, T *p, size_t count) const
    {
        p[0] = T(1); p[count - 1] = T(1);                    // typed stores: the alignment check
        memset((void *)p, 0x5a, count * sizeof(T));          // the whole extent: the bounds check
        printf("blk %s %td %zu %zu\n", name, (char *)p - base, count * sizeof(T), sizeof(T));
    }
};

static void run_case(int nx, int N, int M, int m, int B)
{
    printf("case %d %d %d %d %d\n", nx, N, M, m, B);
    DevCfg c;
    memset(&c, 0, sizeof c);
    c.nx = nx; c.N = N; c.n = 2 * N; c.m = m; c.M = M;
    const size_t Bp = pad64((size_t)B), n = 2 * (size_t)N, mm = m ? m : 1, St = 2 * Bp + 64 * (MPC_MAX_GROUPS + 1);
    {
        Workspace w;
        memset(&w, 0, sizeof w);
        const Arena a("workspace", [&](Carver &k) { workspace_layout(k, w, c, Bp); });
        a.blk("xk", w.xk, n * Bp); a.blk("gk", w.gk, n * Bp); a.blk("q", w.q, n * Bp); a.blk("xn", w.xn, n * Bp);
        a.blk("xe", w.xe, n * Bp); a.blk("ge", w.ge, n * Bp); a.blk("xe2", w.xe2, n * Bp); a.blk("ge2", w.ge2, n * Bp);
        a.blk("S", w.S, M * n * Bp); a.blk("Y", w.Y, M * n * Bp);
        a.blk("Sig", w.Sig, mm * Bp); a.blk("Sig_old", w.Sig_old, mm * Bp); a.blk("e1", w.e1, mm * Bp); a.blk("e2", w.e2, mm * Bp);
        a.blk("yhx", w.yhx, mm * Bp); a.blk("yhxn", w.yhxn, mm * Bp); a.blk("yhe", w.yhe, mm * Bp);
        a.blk("rec", w.rec, REC * Bp);
        a.blk("trajx", w.trajx, (size_t)(N + 1) * nx * St); a.blk("useq", w.useq, 2 * (size_t)N * St);
        a.blk("stage_L", w.stage_L, (size_t)N * St); a.blk("jac", w.jac, (size_t)N * (nx * (nx + 1) + 2) * St);
        a.blk("lists", w.lists, 2 * 2 * Bp); a.blk("agent_of", w.agent_of, St);
        a.blk("counts", w.counts, 8 * MPC_MAX_GROUPS); a.blk("totals", w.totals, 16); a.blk("solo_ctr", w.solo_ctr, 2 * MPC_MAX_GROUPS);
    }
    {
        EventBufs e;
        const Arena a("event", [&](Carver &k) { event_layout(k, e, c, Bp); });
        a.blk("xs", e.xs, nx * Bp); a.blk("Us", e.Us, n * Bp); a.blk("lams", e.lams, mm * Bp);
        a.blk("stats_s", e.stats_s, 8 * Bp); a.blk("stats_own", e.stats_own, 8 * Bp);
        a.blk("list", e.list, Bp); a.blk("fire", e.fire, Bp); a.blk("cis", e.cis, Bp);
        for (int k = 0; k < TAB_KINDS; k++) a.blk(("rows" + std::to_string(k)).c_str(), e.rows[k], Bp);
        a.blk("blk", e.blk, (Bp + EV_BLK - 1) / EV_BLK); a.blk("count", e.count, 64);
    }
    {
        TrafficBufs t;
        const Arena a("traffic", [&](Carver &k) { traffic_layout(k, t, c, Bp); });
        a.blk("X", t.X, (size_t)N * nx * Bp); a.blk("opp", t.opp, MPC_NDISC * Bp);
    }
    {
        ObstacleRuleBufs o;
        const Arena a("obstacle_rule", [&](Carver &k) { obstacle_rule_layout(k, o, Bp); });
        a.blk("clear_chk", o.clear_chk, MPC_NDISC * Bp); a.blk("sel_chk", o.sel_chk, MPC_NDISC * Bp);
    }
    {
        OwnTables o;
        const Arena a("own_tables", [&](Carver &k) { own_tables_layout(k, o, N, Bp); });
        a.blk("ptab", o.ptab, MPC_NPARAM); a.blk("btab", o.btab, MPC_NBOUND); a.blk("rtab", o.rtab, MPC_NRATE);
        a.blk("ftab", o.ftab, MPC_FIELD_ROW(N)); a.blk("pidx", o.pidx, Bp);
    }
}

static void run_grid(int S, int C)
{
    printf("grid %d %d\n", S, C);
    GridBufs g;
    const Arena a("grid", [&](Carver &k) { grid_layout(k, g, (size_t)S, (size_t)C); });
    a.blk("gmeta", g.gmeta, (size_t)GRID_META * C); a.blk("gxy", g.gxy, 2 * (size_t)S * C); a.blk("gcells", g.gcells, (size_t)GRID_CELLS * C);
}

int main()
{
    const int Bs[] = {1, 63, 64, 65, 130, 4096};
    for (int nx : {4, 6})
        for (int N : {1, 20, 64})
            for (int M : {1, N, 64})
                for (int m : {0, N, nx * N, MPC_NDISC * N})
                    for (int B : Bs) run_case(nx, N, M, m, B);
    for (int S : {3, 100})
        for (int C : {1, 5}) run_grid(S, C);
    return 0;
}
