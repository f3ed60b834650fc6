"""Track generators for lap driving (BatchedMPC.track_windows): numpy only, usable without a GPU.

A track row is flat, [x_0..x_{L-1}, y_0..y_{L-1}], like a centerline row (include/mpc_hip.h).  Both tracks here are
CLOSED and do not repeat their first point at the end: point L-1 is followed by point 0.  Both start at the origin
heading along +x and run counter-clockwise, with points equally spaced along the arc.
"""
import numpy as np


def stadium_track(straight, radius, ds):
    """Two straights of length `straight` joined by two half circles of `radius`, about `ds` between points: L =
    round(perimeter / ds) points, exactly perimeter / L apart.  Point 0 is the middle of the lower straight (the origin);
    the upper straight runs along y = 2 radius.  Returns float64 [2L]."""
    straight, radius, ds = float(straight), float(radius), float(ds)
    if not (straight >= 0.0 and radius > 0.0 and ds > 0.0):
        raise ValueError("stadium_track: need straight >= 0, radius > 0 and ds > 0")
    arc = np.pi * radius
    per = 2.0 * straight + 2.0 * arc
    L = int(round(per / ds))
    if L < 4:
        raise ValueError("stadium_track: ds is too large for this track")
    s = (per / L) * np.arange(L)
    h = 0.5 * straight
    x, y = np.empty(L), np.empty(L)
    a = s < h                                           # lower straight, second half
    x[a], y[a] = s[a], 0.0
    b = (s >= h) & (s < h + arc)                        # right half circle, centre (h, radius)
    th = (s[b] - h) / radius
    x[b], y[b] = h + radius * np.sin(th), radius * (1.0 - np.cos(th))
    c = (s >= h + arc) & (s < h + arc + straight)       # upper straight, towards -x
    x[c], y[c] = h - (s[c] - h - arc), 2.0 * radius
    d = (s >= h + arc + straight) & (s < h + 2.0 * arc + straight)   # left half circle, centre (-h, radius)
    th = (s[d] - h - arc - straight) / radius
    x[d], y[d] = -h - radius * np.sin(th), radius * (1.0 + np.cos(th))
    e = s >= h + 2.0 * arc + straight                   # lower straight, first half
    x[e], y[e] = -h + (s[e] - h - 2.0 * arc - straight), 0.0
    return np.concatenate([x, y])


def circle_track(L, radius):
    """L points on a circle of `radius` centred at (0, radius), point 0 at the origin.  Returns float64 [2L]."""
    L, radius = int(L), float(radius)
    if L < 3 or not radius > 0.0:
        raise ValueError("circle_track: need L >= 3 and radius > 0")
    th = 2.0 * np.pi * np.arange(L) / L
    return np.concatenate([radius * np.sin(th), radius * (1.0 - np.cos(th))])
