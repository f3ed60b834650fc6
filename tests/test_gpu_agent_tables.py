"""GPU tests of the host-side logic the three per-agent tables share (mpc_set_agent_params, mpc_set_agent_bounds,
mpc_set_agent_constraints): which entry point refuses a batch size other than the one a bound table is for, and with
which words; that tables bound together are for the same batch; that a null table unbinds.  Every refusal comes before
a kernel of the solve is launched."""
import numpy as np
import pytest
import torch

from agent_tables_common import T
from conftest import straight_centerline, synthetic_states

pytestmark = pytest.mark.gpu

import model_predictive_control_amd as mp  # noqa: E402
from model_predictive_control_amd import _lib  # noqa: E402

N, P, B_BOUND, B_CALL = 8, 2, 64, 32
KINDS = ("params", "bounds", "constraints")
NOUN = dict(params="parameter", bounds="bounds", constraints="constraint")
ROWS = dict(params=_lib.param_rows, bounds=_lib.bound_rows, constraints=_lib.constraint_rows)
ALL = frozenset(KINDS)

# entry point (as the front end names it) -> (the name the library's message begins with, the kinds of table it reads)
ENTRY_POINTS = {
    "rhs": ("mpc_rhs", {"params"}),
    "rollout": ("mpc_rollout", {"params"}),
    "stage_cost": ("mpc_stage_cost", {"params"}),
    "eval_cost_grad": ("mpc_eval_cost_grad", {"params", "constraints"}),
    "eval_cost_grad_wave": ("mpc_eval_cost_grad", {"params", "constraints"}),
    "prox_step": ("mpc_prox_step", {"bounds"}),
    "solve": ("mpc_solve_batch", ALL),
    "solve_async": ("mpc_solve_batch", ALL),
    "solve_active": ("mpc_solve_active", ALL),
    "closed_loop": ("mpc_closed_loop", ALL),
    "closed_loop_event": ("mpc_closed_loop_event", ALL),
    "closed_loop_track": ("mpc_closed_loop_track", ALL),
    "track_locate": ("mpc_track_locate", ALL),
    "track_select": ("mpc_track_select", ALL),
    "stage_errors": ("mpc_stage_errors", set()),
    "lbfgs_apply": ("mpc_lbfgs_apply", set()),
    "lane_payoff": ("mpc_lane_payoff", set()),
    "trigger_eval": ("mpc_trigger_eval", set()),
    "track_windows": ("mpc_track_windows", set()),
    "math_probe": ("mpc_math_probe", set()),
}


class Rig:
    """One engine on which all three tables can be bound, and every entry point called with buffers for B_CALL agents."""

    def __init__(self, dev):
        self.dev = dev
        self.cfg = mp.default_config(mp.MODEL_KINEMATIC, N, constr_mode=_lib.CONSTR_STATE_SQ, max_total_inner=300)
        self.eng = eng = mp.BatchedMPC(self.cfg, dev)
        B, n, M, m = B_CALL, eng.n, eng.M, eng.m
        rng = np.random.default_rng(0)
        z = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device=dev)
        self.x = T(synthetic_states(0, B, seed=1), dev)
        self.cl = T(straight_centerline(), dev)
        self.U = T(np.tile([1., 0.], (B, N)), dev)
        self.u = self.U[:, :2].contiguous()
        self.pose = self.x[:, :3].contiguous()
        self.y, self.Sig = z(B, m), torch.ones(B, m, dtype=torch.float64, device=dev)
        self.gamma = torch.ones(B, dtype=torch.float64, device=dev)
        self.active = torch.ones(B, dtype=torch.int32, device=dev)
        self.held = z(B, dtype=torch.int32)
        self.w = np.ones(eng.nx)
        self.SY = T(rng.uniform(.5, 1.5, (B, M, n)), dev)
        self.zi, self.mask = z(B, dtype=torch.int32), torch.ones(B, n, dtype=torch.float64, device=dev)
        self.ego, self.cars, self.ncars = z(B, 3), z(B, 1, 3), z(B, dtype=torch.int32)
        self.trk = eng.track_windows(self.cl, 1, 0, False)                 # K = 1, L = S: one window
        self.keep = {}

    def call(self, name):
        e, x, cl, U = self.eng, self.x, self.cl, self.U
        if name == "solve_async":
            return e.solve_async(x, cl, U)()
        if name == "eval_cost_grad_wave":
            return e.eval_cost_grad(x, cl, U, self.y, self.Sig, wave=True)
        return {
            "rhs": lambda: e.rhs(x, self.u),
            "rollout": lambda: e.rollout(x, U),
            "stage_cost": lambda: e.stage_cost(x, self.u, cl),
            "eval_cost_grad": lambda: e.eval_cost_grad(x, cl, U, self.y, self.Sig),
            "prox_step": lambda: e.prox_step(U, U, self.gamma),
            "solve": lambda: e.solve(x, cl, U),
            "solve_active": lambda: e.solve_active(x, cl, U, self.active),
            "closed_loop": lambda: e.closed_loop(x, cl, U, 1),
            "closed_loop_event": lambda: e.closed_loop_event(x, cl, U, 1, self.w, 0.0, 3),
            "closed_loop_track": lambda: e.closed_loop_track(x, self.trk, U, 1, self.w, 0.0, 3, self.zi),
            "track_locate": lambda: e.track_locate(x, self.trk),
            "track_select": lambda: e.track_select(x, self.trk, self.zi),
            "stage_errors": lambda: e.stage_errors(self.pose, cl),
            "lbfgs_apply": lambda: e.lbfgs_apply(self.SY, self.SY, self.zi, self.zi, self.mask, U),
            "lane_payoff": lambda: e.lane_payoff(self.ego, self.cars, self.ncars, [1.0] * 15),
            "trigger_eval": lambda: e.trigger_eval(x, x, self.held, self.w, 0.1, 3),
            "track_windows": lambda: e.track_windows(cl, 1, 0, False),
            "math_probe": lambda: e.math_probe(0, self.gamma),
        }[name]()

    def bind(self, kind, B):
        """P rows of the handle's own values for a batch of B agents."""
        self.keep[kind] = (T(ROWS[kind](self.cfg, P), self.dev), T(np.arange(B) % P, self.dev, torch.int32))
        getattr(self.eng, "set_agent_" + kind)(*self.keep[kind])

    def clear(self):
        for kind in KINDS:
            getattr(self.eng, "clear_agent_" + kind)()
        self.keep.clear()


@pytest.fixture(scope="module")
def rig():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    r = Rig(torch.device("cuda:0"))
    yield r
    r.eng.close()


# ----------------------------------------------------------------------------- 1
@pytest.mark.parametrize("kind", KINDS)
def test_refusal_matrix(rig, kind):
    """With one kind of table bound for 64 agents, a call for 32 is refused by exactly the entry points that read that
    kind, in the library's words; unbound, every entry point serves 32."""
    try:
        rig.bind(kind, B_BOUND)
        for name, (who, reads) in ENTRY_POINTS.items():
            if kind not in reads:
                rig.call(name)
                continue
            with pytest.raises(mp.MpcError) as err:
                rig.call(name)
            msg = str(err.value)
            tail = (f": the bound {NOUN[kind]} table is for a batch of {B_BOUND} agents, this call has {B_CALL} "
                    f"(mpc_set_agent_{kind})")
            assert msg.endswith(tail), (name, msg)
            assert msg == f"libmpc_hip error -1: {who}{tail}", (name, msg)    # (the library's message begins with its name)
    finally:
        rig.clear()
    for name in ENTRY_POINTS:
        rig.call(name)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 2
@pytest.mark.parametrize("first,second", [(a, b) for a in KINDS for b in KINDS if a != b])
def test_tables_bound_together_are_for_the_same_batch(rig, first, second):
    try:
        rig.bind(first, B_BOUND)
        with pytest.raises(mp.MpcError, match=f"mpc_set_agent_{second}: the bound {NOUN[first]} table is for a batch of "
                                              f"{B_BOUND} agents$"):
            rig.bind(second, B_CALL)
        assert not getattr(rig.eng, f"agent_{second}_bound")
        rig.bind(first, B_CALL)                 # a table's own earlier binding does not count
        assert getattr(rig.eng, f"agent_{first}_bound")
        rig.bind(second, B_CALL)
        rig.call("solve")
    finally:
        rig.clear()


# ----------------------------------------------------------------------------- 3
@pytest.mark.parametrize("kind", KINDS)
def test_null_table_unbinds_whatever_else_is_passed(rig, kind):
    eng = rig.eng
    fn = getattr(eng.lib, "mpc_set_agent_" + kind)
    idx = rig.zi.data_ptr()

    def unbind(Pn, index, Bn):
        return fn(eng._h, None, Pn, index, *((index,) if kind == "params" else ()), Bn)
    try:
        rig.bind(kind, B_BOUND)
        assert unbind(-3, idx, -7) == 0
        for name in ENTRY_POINTS:               # nothing is bound any more: 32 agents are served
            rig.call(name)
        assert unbind(0, None, 0) == 0 and unbind(5, idx, B_BOUND) == 0
    finally:
        rig.clear()
    torch.cuda.synchronize()
