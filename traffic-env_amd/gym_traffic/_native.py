"""ctypes binding of libtfx_hip.so (include/tfx.h).  There is NO fallback: if the HIP library is
missing or fails to load, importing the env raises - the step path is the GPU kernels or nothing."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TFX_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libtfx_hip.so"))

MAX_ARCH = 64
ACTION_BUFFER, ACTION_BROADCAST, ACTION_CYCLE, ACTION_GREEDY = 0, 1, 2, 3
SPAWN_NONE, SPAWN_COUNTS, SPAWN_PERIODIC = 0, 1, 2
ABI_VERSION = 13
EINVAL, ESTATE = -1, -2                 # TFX_EINVAL, TFX_ESTATE
PERIOD_MAX = 1 << 20                    # TFX_PERIOD_MAX: the longest fixed light cycle
TICK_MAX = 0x7fffffff - PERIOD_MAX      # TFX_TICK_MAX: the clock's domain is 0 .. TICK_MAX
CLONE_STREAM, CLONE_EPISODE = 1, 2      # flags of tfx_clone_envs
MEASURE_ACCUMULATE = 1                  # flag of tfx_road_measures
CELLS_ACCUMULATE = 1                    # flag of tfx_road_cells
MAX_CELLS = 32                          # TFX_MAX_CELLS
TRAVEL_ACCUMULATE = 1                   # flag of tfx_car_ages and tfx_trip_stats
MAX_TRIP_BINS = 32                      # the most bins tfx_trip_stats takes
FRAMES_ROADS_ONLY = 1                   # flag of tfx_frames
FOLLOW_ACCUMULATE = 1                   # flag of tfx_road_following
MAX_HEADS = 16                          # TFX_MAX_HEADS: the most cars tfx_road_ends lists per road
ENDS_NO_CAR = 255                       # TFX_ENDS_NO_CAR: the row of a padded entry
FRAME_PX_MIN, FRAME_PX_MAX = 8, 256     # TFX_FRAME_PX_MIN, TFX_FRAME_PX_MAX
DEMAND_MAX_PROFILES, DEMAND_MAX_SEGMENTS, DEMAND_MAX_CDF = 16, 64, 256   # limits of tfx_set_demand
# TFX_DIGEST_*: the parts of tfx_state_digest
DIGEST_CARS, DIGEST_ROWS, DIGEST_SPAWN, DIGEST_RING, DIGEST_LIGHTS, DIGEST_OBS = 1, 2, 4, 8, 16, 32
DIGEST_ALL = 63


class TfxConfig(C.Structure):
    _fields_ = [("m", C.c_int32), ("n", C.c_int32), ("capacity", C.c_int32), ("n_envs", C.c_int32),
                ("planes", C.c_int32), ("length", C.c_float), ("rate", C.c_float),
                ("car_v", C.c_float), ("car_l", C.c_float), ("car_a", C.c_float),
                ("car_delta", C.c_float), ("car_v0", C.c_float), ("car_b", C.c_float),
                ("car_T", C.c_float), ("car_s0", C.c_float),
                ("yellow_ticks", C.c_int32), ("thresh", C.c_float), ("detect_dist", C.c_float),
                ("overflow_penalty", C.c_float), ("eps", C.c_float),
                ("learn_switch", C.c_int32), ("validate", C.c_int32), ("entry_spec", C.c_uint32),
                ("env_id_offset", C.c_int32), ("layout", C.c_int32),
                ("n_archetypes", C.c_int32), ("arch", (C.c_float * 8) * MAX_ARCH)]


class TfxBuffers(C.Structure):
    _fields_ = [("xv", C.c_void_p), ("w", C.c_void_p), ("leading", C.c_void_p), ("lastcar", C.c_void_p),
                ("obs", C.c_void_p), ("rewards", C.c_void_p), ("waiting", C.c_void_p),
                ("passed_dst", C.c_void_p), ("done_tick", C.c_void_p),
                ("trip_times", C.c_void_p), ("n_trips", C.c_void_p), ("trip_cap", C.c_int32)]


class TfxEpisodeBuffers(C.Structure):
    _fields_ = [("ep_return", C.c_void_p), ("ep_len", C.c_void_p), ("final_return", C.c_void_p),
                ("final_len", C.c_void_p), ("truncated", C.c_void_p), ("ep_index", C.c_void_p)]


class TfxMeasureBuffers(C.Structure):
    _fields_ = [("n_cars", C.c_void_p), ("n_halted", C.c_void_p), ("queue", C.c_void_p), ("speed_sum", C.c_void_p)]


class TfxCellBuffers(C.Structure):
    _fields_ = [("n_cars", C.c_void_p), ("speed_sum", C.c_void_p)]


class TfxAgeBuffers(C.Structure):
    _fields_ = [("n_cars", C.c_void_p), ("age_sum", C.c_void_p), ("age_max", C.c_void_p)]


class TfxTripStatBuffers(C.Structure):
    _fields_ = [("count", C.c_void_p), ("tick_sum", C.c_void_p), ("tick_max", C.c_void_p), ("lost", C.c_void_p),
                ("hist", C.c_void_p)]


class TfxFollowParams(C.Structure):
    _fields_ = [("x_from", C.c_float), ("platoon_gap", C.c_float), ("v_min", C.c_float), ("ttc_crit", C.c_float)]


class TfxFollowBuffers(C.Structure):
    _fields_ = [("n_cars", C.c_void_p), ("n_pairs", C.c_void_p), ("n_joined", C.c_void_p), ("n_overlap", C.c_void_p),
                ("gap_sum", C.c_void_p), ("gap_min", C.c_void_p), ("n_hw", C.c_void_p), ("hw_sum", C.c_void_p),
                ("n_conflict", C.c_void_p), ("ttc_min", C.c_void_p), ("drac_max", C.c_void_p)]


class TfxEndsParams(C.Structure):
    _fields_ = [("k", C.c_int32), ("pad_dist", C.c_float), ("pad_v", C.c_float), ("pad_tail_x", C.c_float)]


class TfxEndsBuffers(C.Structure):
    _fields_ = [("n_cars", C.c_void_p), ("n_heads", C.c_void_p), ("heads", C.c_void_p), ("head_rows", C.c_void_p),
                ("tail", C.c_void_p), ("tail_row", C.c_void_p)]


class TfxCarListBuffers(C.Structure):
    _fields_ = [("xv", C.c_void_p), ("road", C.c_void_p), ("row", C.c_void_p), ("spawn", C.c_void_p)]


class TfxPutBuffers(C.Structure):
    _fields_ = [("xv", C.c_void_p), ("row", C.c_void_p), ("spawn", C.c_void_p), ("leading", C.c_void_p),
                ("lead_x", C.c_void_p)]


class TfxDemand(C.Structure):
    _fields_ = [("n_profiles", C.c_int32), ("n_segments", C.c_int32), ("seg_ticks", C.c_int32),
                ("tick_offset", C.c_int32), ("n_cdf", C.c_int32),
                ("count_cdf", C.c_void_p), ("road_cdf", C.c_void_p), ("profile_of_env", C.c_void_p),
                ("seed", C.c_uint64)]


class TfxError(RuntimeError):
    pass


_lib = None

_PROTOS = {
    "tfx_abi_version": (C.c_int, []),
    "tfx_last_error": (C.c_char_p, []),
    "tfx_create": (C.c_int, [C.POINTER(TfxConfig), C.POINTER(C.c_void_p)]),
    "tfx_destroy": (C.c_int, [C.c_void_p]),
    "tfx_dims": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_int32)] * 4),
    "tfx_tables": (C.c_int, [C.c_void_p] + [C.c_void_p] * 4),
    "tfx_bind_buffers": (C.c_int, [C.c_void_p, C.POINTER(TfxBuffers)]),
    "tfx_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "tfx_reset_envs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tfx_refresh": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tfx_set_episodes": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.POINTER(TfxEpisodeBuffers)]),
    "tfx_set_episode_pool": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tfx_set_actions": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]),
    "tfx_set_spawns": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]),
    "tfx_set_poisson": (C.c_int, [C.c_void_p, C.c_double, C.c_uint64, C.c_void_p, C.c_int32]),
    "tfx_set_regular": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_uint64]),
    "tfx_set_spawn_archetypes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "tfx_set_demand": (C.c_int, [C.c_void_p, C.POINTER(TfxDemand)]),
    "tfx_demand_counts": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "tfx_set_demand_mixed": (C.c_int, [C.c_void_p, C.POINTER(TfxDemand), C.c_void_p, C.c_int32]),
    "tfx_demand_rows": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tfx_demand_rows_per_road": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "tfx_step": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "tfx_move_cars": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tfx_advance_finished_cars": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tfx_agent_step": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tfx_remi": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tfx_cars_on_roads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "tfx_done": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "tfx_get_tick": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "tfx_set_tick": (C.c_int, [C.c_void_p, C.c_int32]),
    "tfx_vehicle_updates": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]),
    "tfx_reset_counters": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tfx_profile": (C.c_int, [C.c_void_p, C.c_int32]),
    "tfx_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "tfx_xv_pairs": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "tfx_export_ring": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tfx_import_ring": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tfx_fastdiv_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "tfx_launch_info": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_int32)] * 3),
    "tfx_arrivals_replay": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "tfx_arrivals_replay_rows": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                                           C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_int32, C.c_int32, C.c_void_p]),
    "tfx_fused_ticks": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "tfx_pair_ticks": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "tfx_tail_ticks": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "tfx_slow_pairs": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]),
    "tfx_split_ticks": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "tfx_step_kernel": (C.c_char_p, [C.c_void_p]),
    "tfx_debug_fail_after": (C.c_int, [C.c_void_p, C.c_int32]),
    "tfx_clone_envs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "tfx_clone_skipped": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]),
    "tfx_debug_head_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "tfx_road_measures": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.POINTER(TfxMeasureBuffers), C.c_int32, C.c_void_p]),
    "tfx_measure_launch": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tfx_road_cells": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.POINTER(TfxCellBuffers), C.c_int32, C.c_void_p]),
    "tfx_cells_launch": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tfx_car_ages": (C.c_int, [C.c_void_p, C.POINTER(TfxAgeBuffers), C.c_int32, C.c_void_p]),
    "tfx_ages_launch": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tfx_trip_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.POINTER(TfxTripStatBuffers),
                                 C.c_int32, C.c_void_p]),
    "tfx_frame_size": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tfx_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "tfx_frames_launch": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tfx_road_following": (C.c_int, [C.c_void_p, C.POINTER(TfxFollowParams), C.POINTER(TfxFollowBuffers), C.c_int32,
                                     C.c_void_p]),
    "tfx_follow_launch": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tfx_road_ends": (C.c_int, [C.c_void_p, C.POINTER(TfxEndsParams), C.POINTER(TfxEndsBuffers), C.c_int32, C.c_void_p]),
    "tfx_ends_launch": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tfx_car_list": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                               C.POINTER(TfxCarListBuffers), C.c_int32, C.c_void_p]),
    "tfx_car_list_launch": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tfx_put_cars": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                               C.POINTER(TfxPutBuffers), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "tfx_put_launch": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tfx_state_digest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_int32, C.c_void_p]),
    "tfx_digest_launch": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
}


def lib():
    """The loaded library; raises TfxError if it is absent (no CPU fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TfxError("HIP library not found at %s - build it with `python -c 'import "
                           "__graft_entry__ as g; g.build()'` (or make -C traffic-env_amd/csrc). "
                           "There is no CPU fallback for the env step." % LIB_PATH)
        try:
            handle = C.CDLL(LIB_PATH)
        except OSError as exc:
            raise TfxError("cannot load %s: %s" % (LIB_PATH, exc))
        for name, (res, argtypes) in _PROTOS.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = argtypes
        if handle.tfx_abi_version() != ABI_VERSION:
            raise TfxError("libtfx_hip.so ABI %d != binding ABI %d" % (handle.tfx_abi_version(), ABI_VERSION))
        _lib = handle
    return _lib


def check(rc):
    if rc != 0:
        raise TfxError("tfx error %d: %s" % (rc, lib().tfx_last_error().decode("utf-8", "replace")))
    return rc
