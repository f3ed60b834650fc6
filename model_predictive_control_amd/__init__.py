"""MI355X-native batched MPC solve step (drop-in for panagiotou23/model-predictive-control's
controller.MPCController hot path).  Host code is Python; kernels are hand-written HIP for gfx950
behind the C-ABI in include/mpc_hip.h."""
from . import _lib
from ._lib import (MODEL_KINEMATIC, MODEL_PACEJKA, WRAP_FLOOR, WRAP_FMOD, WRAP_IEEE, CONSTR_NONE,
                   CONSTR_STATE_SQ, CONSTR_LANE, CONSTR_DISCS, NDISC, SCENE_MAX, default_discs, disc_rows,
                   NRATE, default_rates, rate_rows, NFIELD, NFSRC, field_row, default_fields, field_rows,
                   NSTATS, NPARAM, MpcConfig, default_config, default_params, param_rows, NBOUND,
                   default_bounds, bound_rows, NCONSTR, default_constraints, constraint_rows, MpcError,
                   obstacle_tracks, obstacle_width, NROAD, default_roads, road_rows)
from .solver import BatchedMPC, Track, TrafficLoopResult, ObstacleLoopResult, ObstacleEventLoopResult, TrafficEventLoopResult
from .tracks import stadium_track, circle_track

__all__ = ["BatchedMPC", "MpcConfig", "default_config", "MpcError", "MODEL_KINEMATIC", "MODEL_PACEJKA",
           "WRAP_FLOOR", "WRAP_FMOD", "WRAP_IEEE", "CONSTR_NONE", "CONSTR_STATE_SQ", "CONSTR_LANE",
           "CONSTR_DISCS", "NDISC", "SCENE_MAX", "default_discs", "disc_rows", "NRATE", "default_rates",
           "rate_rows", "NFIELD", "NFSRC", "field_row", "default_fields", "field_rows", "NSTATS", "NPARAM",
           "default_params", "param_rows", "NBOUND", "default_bounds", "bound_rows", "NCONSTR",
           "default_constraints", "constraint_rows", "Track", "TrafficLoopResult", "stadium_track",
           "circle_track", "ObstacleLoopResult", "ObstacleEventLoopResult", "obstacle_tracks", "obstacle_width", "NROAD",
           "default_roads", "road_rows", "TrafficEventLoopResult"]
