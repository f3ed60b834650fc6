"""CPU tests of lap driving (no GPU): mpc_track_init's counts and refusals through the library, the property the select
rule is built for -- where nothing is clamped the nearest index on the new row lies in [lead, lead + w) --, the track
generators, and the conditions of the oracle mirror across the seam that tests/test_gpu_track_loop.py compares the
MI355X with (tests/track_loop_common.py)."""
import ctypes as C

import numpy as np
import pytest

import track_loop_common as K

import model_predictive_control_amd as mp
from model_predictive_control_amd import _lib
from model_predictive_control_amd.tracks import stadium_track, circle_track


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.load()


def test_exports_and_argtypes(L):
    vp, ci, tp = C.c_void_p, C.c_int, C.POINTER(_lib.MpcTrack)
    for name in ("mpc_track_init", "mpc_track_windows", "mpc_track_locate", "mpc_track_select", "mpc_closed_loop_track"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).restype is ci
    assert L.mpc_track_init.argtypes == [tp, C.POINTER(_lib.MpcConfig)] + [ci] * 5
    assert L.mpc_track_windows.argtypes == [vp, tp, vp, vp, vp]
    assert L.mpc_track_locate.argtypes == [vp, tp, ci] + [vp] * 5
    assert L.mpc_track_select.argtypes == [vp, tp, ci] + [vp] * 6
    assert L.mpc_closed_loop_track.argtypes == L.mpc_closed_loop_event.argtypes + [tp, vp]
    assert C.sizeof(_lib.MpcTrack) == 24 and [f[0] for f in _lib.MpcTrack._fields_] == ["K", "L", "stride", "lead", "closed", "R"]
    assert "Track" in mp.__all__ and "stadium_track" in mp.__all__ and "circle_track" in mp.__all__


@pytest.mark.parametrize("S", [100, 37])
def test_track_init_counts(L, S):
    cfg = mp.default_config(0, 20, S=S)
    for K_, Ln, w, lead, closed in [(1, S, 1, 0, 0), (1, S, 7, 3, 0), (1, S, 7, 3, 1), (3, 388, 4, 10, 1), (3, 389, 4, 10, 1),
                                    (2, 400, 4, 10, 0), (2, 401, 50, S - 2, 0), (1, 1000, 1, 0, 1), (1, 1000, 2000, 5, 1),
                                    (1, 1000, 2000, 5, 0), (1, S + 1, 1, 0, 0), (5, 100000, 3, 1, 1)]:
        t = _lib.track_init(cfg, K_, Ln, w, lead, closed)
        g = K.geom(K_, Ln, S, w, lead, closed)
        assert (t.K, t.L, t.stride, t.lead, t.closed, t.R) == (K_, Ln, w, lead, int(closed), g.R)
        assert t.R == (-(-Ln // w) if closed else (Ln - S) // w + 1)
        if not closed:                                    # the last window ends inside the track
            assert (t.R - 1) * w + S - 1 <= Ln - 1
    assert _lib.track_init(cfg, 1, S, 1, 0, 0).R == 1         # L = S: one window
    assert _lib.track_init(cfg, 1, 388, 4, 10, 1).R == 97     # the seam case


def test_track_init_refusals(L):
    cfg = mp.default_config(0, 20)                            # S = 100
    t = _lib.MpcTrack()
    ok = dict(K=1, L=388, stride=4, lead=10, closed=1)
    for bad in (dict(K=0), dict(K=-1), dict(L=99), dict(L=0), dict(stride=0), dict(stride=-4), dict(lead=-1), dict(lead=99),
                dict(K=2 ** 30, L=2 ** 20, stride=1), dict(K=2 ** 24, L=2 ** 20, stride=1, closed=0)):
        a = dict(ok, **bad)
        rc = L.mpc_track_init(C.byref(t), C.byref(cfg), a["K"], a["L"], a["stride"], a["lead"], a["closed"])
        assert rc == -1 and L.mpc_last_error().decode().startswith("mpc_track_init"), bad
        with pytest.raises(ValueError):
            _lib.track_init(cfg, a["K"], a["L"], a["stride"], a["lead"], a["closed"])
    assert L.mpc_track_init(None, C.byref(cfg), 1, 388, 4, 10, 1) == -1
    assert L.mpc_track_init(C.byref(t), None, 1, 388, 4, 10, 1) == -1
    assert L.mpc_track_init(C.byref(t), C.byref(cfg), 1, 388, 4, 98, 1) == 0          # lead = S - 2 is the last allowed
    assert L.mpc_track_init(C.byref(t), C.byref(cfg), 2047, 2 ** 20, 1, 0, 1) == 0 and t.R == 2 ** 20   # K R < 2^31
    # the calls that take a handle refuse a null one (and a null track) without touching a device
    assert L.mpc_track_windows(None, C.byref(t), None, None, None) == -1
    assert L.mpc_track_select(None, C.byref(t), 4, None, None, None, None, None, None) == -1
    assert L.mpc_track_locate(None, C.byref(t), 4, None, None, None, None, None) == -1
    w4 = (C.c_double * 4)(1, 1, 1, 1)
    held = (C.c_int32 * 4)()
    assert L.mpc_closed_loop_track(None, 4, 1, 0, w4, 0.0, 1, None, None, None, None, None, held, None, None, None, None,
                                   None, None, None, None, None, None) == -1
    assert "null track" in L.mpc_last_error().decode()
    assert L.mpc_closed_loop_track(None, 4, 1, 0, w4, 0.0, 1, None, None, None, None, None, held, None, None, None, None,
                                   None, None, None, None, C.byref(t), None) == -1
    assert "null handle" in L.mpc_last_error().decode()


def test_track_generators():
    tr = stadium_track(10, 3, 0.1)
    Ln = tr.size // 2
    assert Ln == 388 and tr[0] == 0.0 and tr[Ln] == 0.0                    # point 0: the origin, mid-straight
    x, y = tr[:Ln], tr[Ln:]
    step = np.hypot(np.diff(np.r_[x, x[0]]), np.diff(np.r_[y, y[0]]))      # the closing step included: no repeated point
    per = 2 * 10 + 2 * np.pi * 3
    assert step.min() > 0.9 * per / Ln and step.max() <= per / Ln * (1 + 1e-12)
    assert x[1] > 0 and y[1] == 0 and x[-1] < 0 and y[-1] == 0 and abs(y.max() - 6) < 1e-3 and abs(x.max() - 8) < 1e-3
    c = circle_track(50, 2.0)
    assert c.shape == (100,) and c[0] == 0 and c[50] == 0
    assert np.allclose(np.hypot(c[:50], c[50:] - 2.0), 2.0, rtol=0, atol=1e-15)
    d = np.hypot(np.diff(np.r_[c[:50], c[0]]), np.diff(np.r_[c[50:], c[50]]))
    assert np.allclose(d, d[0], rtol=1e-12)
    for bad in (lambda: stadium_track(10, 0, 0.1), lambda: stadium_track(10, 3, 0), lambda: circle_track(2, 1.0)):
        with pytest.raises(ValueError):
            bad()


def test_windows_are_a_gather():
    tr = np.stack([stadium_track(10, 3, 0.1), stadium_track(10, 3, 0.1) + 1.0])
    for closed, S, w in [(True, 100, 4), (True, 37, 5), (False, 100, 7), (False, 37, 1)]:
        g = K.geom(2, 388, S, w, 3, closed)
        win = K.windows(tr, g)
        assert win.shape == (2 * g.R, 2 * S)
        for k, r, i in [(0, 0, 0), (1, g.R - 1, S - 1), (1, g.R // 2, 5), (0, g.R - 1, 0)]:
            p = r * w + i
            p = p % 388 if closed else p
            assert win[k * g.R + r, i] == tr[k, p] and win[k * g.R + r, S + i] == tr[k, 388 + p]


@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("S,w,lead", [(100, 4, 10), (37, 5, 3), (100, 1, 0), (100, 30, 60)])
def test_select_puts_the_nearest_index_into_the_lead_band(O, closed, S, w, lead):
    """Where select is not clamped, the nearest index on the new row lies in [lead, lead + w), and selecting again from
    the new row changes nothing.  Poses within 3 cm of a track point (a third of the spacing: that point is the nearest
    of any window that holds it among its candidates)."""
    tr = stadium_track(10, 3, 0.1)
    Ln = tr.size // 2
    g = K.geom(1, Ln, S, w, lead, closed)
    assert lead + w - 1 <= S - 2                             # the band lies among a row's candidates 0 .. S-2
    win = K.windows(tr, g)
    cfg = O.default_config(0, 20, S=S)
    rng = np.random.default_rng(3)
    n = 0
    for _ in range(300):
        r, i = int(rng.integers(0, g.R)), int(rng.integers(0, S - 1))
        pt = np.array([win[r, i], win[r, S + i]]) + rng.uniform(-0.03, 0.03, 2)
        rows, pos = K.select(O, cfg, pt[None, :], win, [r], g)
        assert pos[0] == ((r * w + i) % Ln if closed else r * w + i)
        if not closed and not 0 <= (pos[0] - lead) // w <= g.R - 1:
            assert rows[0] in (0, g.R - 1)                   # clamped: the first or the last window
            continue
        j = O.nearest(cfg, pt, win[rows[0]])
        assert lead <= j < lead + w, (r, i, int(rows[0]), j)
        assert j == ((pos[0] - rows[0] * w) % Ln if closed else pos[0] - rows[0] * w)
        rows2, pos2 = K.select(O, cfg, pt[None, :], win, rows, g)
        assert rows2[0] == rows[0] and pos2[0] == pos[0]
        n += 1
    assert n > (250 if closed else 100)


@pytest.mark.parametrize("model,N", K.SEAM_MODELS)
@pytest.mark.parametrize("thr", K.SEAM_THRESHOLDS)
def test_seam_case_satisfies_its_conditions(O, model, N, thr):
    """The conditions of the oracle mirror across the seam, on the oracle alone: no failed solve, at least one seam
    crossing, and no selection closer than 1e-4 (relative gap of the two nearest squared distances) to choosing another
    index -- two implementations' states differ by about 1e-9.  Under eval_jitter(2, 5) the rows are identical."""
    ref = K.seam_mirror(O, model, N, thr)
    jit = K.seam_mirror(O, model, N, thr, jitter=(2, 5))
    dx = np.abs(ref["traj_x"] - jit["traj_x"]).max()
    print(f"model {model} thr {thr}: solves {int(ref['solved'].sum())}, failed {int(ref['fails'].sum())}, row changes "
          f"{ref['row_changes']}, seam crossings {ref['seam_crossings']}, gap {ref['gap']:.2e}, margin {ref['margin']:.2e}, "
          f"jittered states within {dx:.2e}")
    assert ref["fails"].sum() == 0
    assert ref["seam_crossings"] >= 1
    assert ref["gap"] > 1e-4
    if thr > 0:
        assert ref["margin"] > 1e-3                       # (as tests/test_event_loop_cpu.py asks of the trigger's decisions)
        assert 0.05 < ref["solved"].mean() < 0.9
    assert np.array_equal(ref["traj_row"], jit["traj_row"]) and np.array_equal(ref["solved"], jit["solved"])
