"""ctypes binding of libagz.so (include/agz.h).  No compute happens in Python and nothing here falls
back to the CPU: if the HIP library or a GPU is missing, calls raise AgzError."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# constants from include/agz.h
NONE, BLACK, WHITE = 0, 1, 2
PASS, RESIGN = -1, -2
NO_MOVE = -32768
GAME_MNK, GAME_C4, GAME_KOMI, GAME_WQ = 0, 1, 2, 3
ENC_TWOPLANE, ENC_WQ = 0, 1
INF_NET, INF_DUMMY, INF_SCRIPT, INF_HASH, INF_UNIFORM, INF_CALLBACK = 0, 1, 2, 3, 4, 5
BN_DEGENERATE_EPS, BN_RUNNING, BN_IDENTITY = 0, 1, 2
COMPUTE_F32_MFMA, COMPUTE_BF16X3, COMPUTE_FP16X2, COMPUTE_WINO, COMPUTE_AUTO, COMPUTE_WINO_H2 = 0, 1, 2, 3, 4, 5
COMPUTE_FORCE = 0x100
LOSS_REFERENCE, LOSS_ALPHAZERO = 0, 1   # agz_trainer_set_loss
# agz_debug.h, agz_trainer_last_paths: the kernel a trainer layer's last step took (0 = none launched)
PATH_FWD_F32, PATH_FWD_BF16X3, PATH_FWD_H2W, PATH_FWD_H2DMA, PATH_FWD_H2DMA3 = 1, 2, 3, 4, 5
PATH_WGRAD_F32, PATH_WGRAD_X3, PATH_WGRAD_H2, PATH_WGRAD_H2T3 = 1, 2, 3, 4
PATH_DGRAD_RAW, PATH_DGRAD_X3, PATH_DGRAD_WINO_H2 = 1, 2, 3
PATH_BN2_SCALAR, PATH_BN2_V = 1, 2
# agz_debug.h, agz_trainer_last_rows: the words of a tower layer's row plan, and of the heads' (layer SharedLayers + 1)
ROWS_WGRAD_CHUNKS, ROWS_SINGLE_PASS, ROWS_APPLY_RPB, ROWS_BWD2_RPB = 0, 1, 2, 3
ROWS_APPLY_BOARD_WORDS, ROWS_BWD2_BOARD_WORDS, ROWS_SPLIT_BLOCKS, ROWS_SPLIT_NEED = 4, 5, 6, 7
ROWS_HEAD_SECOND_FORM, ROWS_HEAD_CONV2_GRID, ROWS_HEAD_STATS_GRID, ROWS_HEAD_COST_GRID = 0, 1, 2, 3
# agz_debug.h, agz_net_last_paths: the kernels a net's last whole-batch forward launched (0 = none)
NPATH_IN_LAT, NPATH_IN_X3, NPATH_IN_F32_411, NPATH_IN_F32_221, NPATH_IN_F32_222 = 1, 2, 3, 4, 5
NPATH_BLK_F32_411, NPATH_BLK_F32_221, NPATH_BLK_F32_222 = 1, 2, 3
NPATH_BLK_F32_411_SPLITK, NPATH_BLK_F32_221_SPLITK, NPATH_BLK_F32_222_SPLITK = 4, 5, 6
NPATH_BLK_X3, NPATH_BLK_H2W, NPATH_BLK_H2, NPATH_BLK_WINO = 7, 8, 9, 10
NPATH_BLK_WINO_H2_3K, NPATH_BLK_WINO_H2_3K_WIDE, NPATH_BLK_WINO_H2_CHAINED, NPATH_BLK_LAT_H2 = 11, 12, 13, 14
NPATH_HEADS_ONE, NPATH_HEADS_SPREAD, NPATH_HEADS_SPREAD_NB4 = 1, 2, 3
PROF_CONV, PROF_HEADS, PROF_SELECT, PROF_EXPAND, PROF_MOVE, PROF_CONV_INIT = 0, 1, 2, 3, 4, 5
PROF_WINO_IN, PROF_WINO_GEMM, PROF_WINO_OUT = 6, 7, 8
DONT_PREFER_PASS, PREFER_PASS, DONT_RESIGN = 0, 1, 2
POOL_STRICT, POOL_STOP_SEARCH, POOL_GROW = 0, 1, 2
SYM_OFF, SYM_RANDOM, SYM_FIXED = 0, 1, 8   # set_leaf_symmetry: SYM_FIXED + k applies S_k at every leaf
TARGET_REFERENCE, TARGET_VISITS = 0, 1     # Arena.set_policy_target
CAP_FULL, CAP_FAST = 0, 1                  # Arena.playout_cap / playout_cap_of


class AgzError(RuntimeError):
    pass


class NetConf(C.Structure):
    """agz_net_conf == dual.Config (dualnet/config.go:4-16)."""
    _fields_ = [("K", C.c_int32), ("SharedLayers", C.c_int32), ("FC", C.c_int32), ("BatchSize", C.c_int32),
                ("Width", C.c_int32), ("Height", C.c_int32), ("Features", C.c_int32), ("ActionSpace", C.c_int32),
                ("bn_mode", C.c_int32), ("bn_eps", C.c_float)]


class SolverConf(C.Structure):
    """agz_solver_conf: the options of gorgonia's solver constructor (dualnet/meta.go:20) — momentum, WithL2Reg, WithClip; all 0 = vanilla."""
    _fields_ = [("momentum", C.c_float), ("l2reg", C.c_float), ("clip", C.c_float), ("reserved", C.c_int32)]


class AdamConf(C.Structure):
    """agz_adam_conf: gorgonia.NewAdamSolver's options (dualnet/meta.go:20) — beta1, beta2, eps; on = 0 / 1."""
    _fields_ = [("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("on", C.c_int32)]


class GameConf(C.Structure):
    _fields_ = [("kind", C.c_int32), ("m", C.c_int32), ("n", C.c_int32), ("k", C.c_int32), ("komi", C.c_float),
                ("max_moves", C.c_int32), ("encoder", C.c_int32)]


class MctsConf(C.Structure):
    """agz_mcts_conf == mcts.Config (mcts/tree.go:15-29), Timeout -> Budget simulations."""
    _fields_ = [("PUCT", C.c_float), ("M", C.c_int32), ("N", C.c_int32), ("RandomCount", C.c_int32),
                ("Budget", C.c_int32), ("RandomMinVisits", C.c_uint32), ("RandomTemperature", C.c_float),
                ("DumbPass", C.c_int32), ("ResignPercentage", C.c_float), ("PassPreference", C.c_int32)]


class NoiseConf(C.Structure):
    """agz_noise_conf (include/agz.h): root noise P = (1 - eps) p + eps eta, eta ~ Dir(alpha); 16 bytes"""
    _fields_ = [("eps", C.c_float), ("alpha", C.c_float), ("on", C.c_int32), ("reserved", C.c_int32)]


class TargetConf(C.Structure):
    """agz_target_conf (include/agz.h): what an arena records as an example's policy row; 16 bytes"""
    _fields_ = [("kind", C.c_int32), ("temperature", C.c_float), ("reserved", C.c_int32 * 2)]


class PlayoutCapConf(C.Structure):
    """agz_playout_cap_conf (include/agz.h): every ply a FULL search with probability p_full, else fast_budget simulations; 24 bytes"""
    _fields_ = [("p_full", C.c_float), ("fast_budget", C.c_int32), ("on", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64)]


class ForcedConf(C.Structure):
    """agz_forced_conf (include/agz.h): forced playouts at the root with coefficient k, and the pruned policy target; 16 bytes"""
    _fields_ = [("k", C.c_float), ("on", C.c_int32), ("prune", C.c_int32), ("reserved", C.c_int32)]


class ArenaStats(C.Structure):
    _fields_ = [("sims_total", C.c_int64), ("sims_nonnull", C.c_int64), ("nn_evals", C.c_int64),
                ("moves_played", C.c_int64), ("games_finished", C.c_int64), ("examples", C.c_int64),
                ("n_games", C.c_int32), ("n_active", C.c_int32), ("tree_full", C.c_int32), ("examples_dropped", C.c_int32),
                ("path_nodes", C.c_int64), ("children_read", C.c_int64)]


class State(C.Structure):
    """agz_state: a host-side game.State handed to mcts.SetGame (include/agz.h)."""
    _fields_ = [("board", C.POINTER(C.c_int32)), ("to_move", C.c_int32), ("n_moves", C.c_int32), ("passes", C.c_int32),
                ("hash", C.c_uint32), ("captures_black", C.c_float), ("captures_white", C.c_float),
                ("last_moves", C.POINTER(C.c_int32)), ("n_last_moves", C.c_int32),
                ("historical", C.POINTER(C.c_int32)), ("n_historical", C.c_int32)]


class GameState(C.Structure):
    _fields_ = [("to_move", C.c_int32), ("move_number", C.c_int32), ("passes", C.c_int32), ("ended", C.c_int32),
                ("winner", C.c_int32), ("a_is_black", C.c_int32), ("last_move", C.c_int32), ("reserved", C.c_int32),
                ("score_black", C.c_float), ("score_white", C.c_float)]


class LeafBatch(C.Structure):
    """agz_leaf_batch (include/agz.h): the leaves a host inferencer (AGZ_INF_CALLBACK) is handed in one call"""
    _fields_ = [("n", C.c_int32), ("features", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("policy_len", C.c_int32),
                ("planes", C.POINTER(C.c_float)), ("board", C.POINTER(C.c_int32)), ("to_move", C.POINTER(C.c_int32)),
                ("move_number", C.POINTER(C.c_int32)), ("game", C.POINTER(C.c_int32)), ("policy", C.POINTER(C.c_float)),
                ("value", C.POINTER(C.c_float))]


INFER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(LeafBatch))


def make_infer_fn(py):
    """agz_infer_fn around a Python function  leaves -> (policy [n, policy_len], value [n]);  leaves = dict(planes [n, F, H, W], board
    [n, H*W], to_move [n], move_number [n], game [n]).  An exception inside `py` is reported to libagz as a failed call (the search aborts
    with AGZ_E_CALLBACK) and re-raised by the binding afterwards."""
    box = {"exc": None}

    def tramp(_user, bp):
        try:
            b = bp.contents
            n, F, H, W, pl = b.n, b.features, b.height, b.width, b.policy_len
            as_np = np.ctypeslib.as_array
            leaves = {"planes": as_np(b.planes, shape=(n, F, H, W)), "board": as_np(b.board, shape=(n, H * W)),
                      "to_move": as_np(b.to_move, shape=(n,)), "move_number": as_np(b.move_number, shape=(n,)),
                      "game": as_np(b.game, shape=(n,)), "policy_len": pl}
            pol, val = py(leaves)
            as_np(b.policy, shape=(n, pl))[...] = np.asarray(pol, np.float32).reshape(n, pl)
            as_np(b.value, shape=(n,))[...] = np.asarray(val, np.float32).reshape(n)
            return 0
        except BaseException as e:   # never let an exception unwind through the C frames
            box["exc"] = e
            return 1

    fn = INFER_FN(tramp)
    fn._box = box
    return fn


def lib_path():
    return os.environ.get("AGZ_LIB_PATH") or os.path.join(_HERE, "lib", "libagz.so")


def lib():
    """Load libagz.so (built in-tree by `make` / __graft_entry__.build())."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise AgzError("libagz.so not built (%s): run `make` or __graft_entry__.build(); there is no CPU fallback"
                       % path)
    L = C.CDLL(path)
    vp, i32, u64, f64 = C.c_void_p, C.c_int, C.c_uint64, C.c_double
    pvp = C.POINTER(C.c_void_p)
    pf, pi, pu, pu8 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)

    def sig(name, res, *args):
        f = getattr(L, name)
        f.restype = res
        f.argtypes = list(args)

    sig("agz_last_error", C.c_char_p)
    sig("agz_version", C.c_char_p)
    sig("agz_ctx_create", i32, i32, pvp)
    sig("agz_ctx_destroy", None, vp)
    sig("agz_ctx_sync", i32, vp)
    sig("agz_ctx_stream", vp, vp)
    sig("agz_ctx_prof_enable", i32, vp, i32)
    sig("agz_ctx_prof_read", i32, vp, i32, C.POINTER(C.c_int64), C.POINTER(C.c_double))
    sig("agz_net_create", i32, vp, C.POINTER(NetConf), pvp)
    sig("agz_net_destroy", None, vp)
    sig("agz_net_num_params", i32, vp)
    sig("agz_net_param_info", i32, vp, i32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t))
    sig("agz_net_set_param", i32, vp, i32, pf, C.c_size_t)
    sig("agz_net_get_param", i32, vp, i32, pf, C.c_size_t)
    sig("agz_net_set_bn_stats", i32, vp, i32, pf, pf, C.c_size_t)
    sig("agz_net_init_random", i32, vp, u64)
    sig("agz_net_commit", i32, vp)
    sig("agz_net_infer", i32, vp, pf, i32, pf, pf)
    sig("agz_net_infer_dev", i32, vp, vp, i32, vp, vp)
    sig("agz_host_alloc", i32, vp, C.c_size_t, pvp)
    sig("agz_host_free", i32, vp, vp)
    sig("agz_mcts_to_dot", i32, vp, i32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t))
    sig("agz_mcts_set_timeout_ms", i32, vp, i32)
    sig("agz_mcts_last_simulations", i32, vp, C.POINTER(C.c_int64))
    sig("agz_net_set_latency_mode", i32, vp, i32)
    sig("agz_net_set_tower_queues", i32, vp, i32)
    sig("agz_net_set_compute_mode", i32, vp, i32)
    sig("agz_net_flops_per_eval", f64, vp)
    sig("agz_net_save", i32, vp, C.c_char_p)
    sig("agz_net_load", i32, vp, C.c_char_p)
    sig("agz_arena_get_results", i32, vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64))
    sig("agz_trainer_create", i32, vp, C.POINTER(NetConf), pvp)
    sig("agz_trainer_create_tied", i32, vp, C.POINTER(NetConf), pvp)
    sig("agz_trainer_is_tied", i32, vp, C.POINTER(i32))
    sig("agz_trainer_destroy", None, vp)
    sig("agz_trainer_num_params", i32, vp)
    sig("agz_trainer_param_info", i32, vp, i32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t))
    sig("agz_trainer_set_param", i32, vp, i32, pf, C.c_size_t)
    sig("agz_trainer_get_param", i32, vp, i32, pf, C.c_size_t)
    sig("agz_trainer_get_grad", i32, vp, i32, pf, C.c_size_t)
    sig("agz_trainer_init_random", i32, vp, u64)
    sig("agz_trainer_batch", i32, vp, pf, pf, pf, C.c_float, pf)
    sig("agz_trainer_forward_backward", i32, vp, pf, pf, pf, pf)
    sig("agz_trainer_forward_backward_dev", i32, vp, vp, vp, vp, pf)
    sig("agz_trainer_apply", i32, vp, C.c_float, C.c_float)
    sig("agz_trainer_grads_dev", i32, vp, pvp, C.POINTER(C.c_size_t))
    sig("agz_trainer_set_solver", i32, vp, C.POINTER(SolverConf))
    sig("agz_trainer_get_solver", i32, vp, C.POINTER(SolverConf))
    sig("agz_trainer_get_velocity", i32, vp, i32, pf, C.c_size_t)
    sig("agz_trainer_set_velocity", i32, vp, i32, pf, C.c_size_t)
    sig("agz_trainer_reset_solver", i32, vp)
    sig("agz_trainer_set_adam", i32, vp, C.POINTER(AdamConf))
    sig("agz_trainer_get_adam", i32, vp, C.POINTER(AdamConf), C.POINTER(C.c_uint64))
    sig("agz_trainer_get_moments", i32, vp, i32, pf, pf, C.c_size_t)
    sig("agz_trainer_set_moments", i32, vp, i32, pf, pf, C.c_size_t)
    sig("agz_trainer_set_bn_tracking", i32, vp, i32, C.c_float)
    sig("agz_trainer_get_bn_tracking", i32, vp, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double))
    sig("agz_trainer_num_bn", i32, vp)
    sig("agz_trainer_get_bn_stats", i32, vp, i32, pf, pf, C.c_size_t)
    sig("agz_trainer_set_bn_stats", i32, vp, i32, pf, pf, C.c_size_t, C.c_double)
    sig("agz_trainer_reset_bn_stats", i32, vp)
    sig("agz_trainer_eval", i32, vp, pf, pf, pf, pf)
    sig("agz_trainer_eval_dev", i32, vp, vp, vp, vp, pf)
    sig("agz_trainer_set_loss", i32, vp, i32)
    sig("agz_trainer_get_loss", i32, vp, C.POINTER(C.c_int))
    sig("agz_trainer_get_costs", i32, vp, pf, pf)
    sig("agz_trainer_set_compute_mode", i32, vp, i32)
    sig("agz_train", i32, vp, pf, pf, pf, i32, i32, u64, pf)
    sig("agz_trainer_export", i32, vp, vp)
    sig("agz_trainer_save", i32, vp, C.c_char_p)
    sig("agz_trainer_load", i32, vp, C.c_char_p)
    sig("agz_arena_create", i32, vp, C.POINTER(GameConf), C.POINTER(MctsConf), i32, u64, i32, pvp)
    sig("agz_arena_destroy", None, vp)
    sig("agz_arena_set_inferencer", i32, vp, i32, i32, vp)
    sig("agz_arena_reset", i32, vp, pu8)
    sig("agz_arena_play", i32, vp, i32, i32)
    sig("agz_arena_selfplay", i32, vp, C.c_int64, i32)
    sig("agz_arena_set_parallel", i32, vp, i32)
    sig("agz_arena_set_leaf_symmetry", i32, vp, i32, u64)
    sig("agz_mcts_set_leaf_symmetry", i32, vp, i32, u64)
    sig("agz_symmetry_map", i32, i32, i32, pi)
    sig("agz_symmetry_inverse", i32, i32)
    sig("agz_leaf_symmetry_of", i32, u64, pi, i32, i32, C.POINTER(C.c_int))
    sig("agz_examples_augment_dihedral", i32, vp)
    sig("agz_symmetry_boards", i32, vp, pf, i32, i32, i32, pf)
    pnc, pu64 = C.POINTER(NoiseConf), C.POINTER(C.c_uint64)
    sig("agz_arena_set_root_noise", i32, vp, pnc)
    sig("agz_arena_get_root_noise", i32, vp, pnc)
    sig("agz_arena_root_noise", i32, vp, i32, i32, pu64, pi, pf, i32, C.POINTER(C.c_int))
    sig("agz_mcts_set_root_noise", i32, vp, pnc)
    sig("agz_mcts_root_noise", i32, vp, pu64, pi, pf, i32, C.POINTER(C.c_int))
    sig("agz_root_noise_of", i32, u64, i32, C.c_float, pf)
    ppc, pi32, pi64 = C.POINTER(PlayoutCapConf), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    sig("agz_arena_set_playout_cap", i32, vp, ppc)
    sig("agz_arena_get_playout_cap", i32, vp, ppc)
    sig("agz_arena_playout_cap", i32, vp, i32, pu64, pi32, pi32, pi32)
    sig("agz_arena_playout_cap_counts", i32, vp, pi64, pi64)
    sig("agz_playout_cap_of", i32, u64, u64, C.c_int32, C.c_float, pi32)
    pfc, pu8, pu32 = C.POINTER(ForcedConf), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    sig("agz_arena_set_forced_playouts", i32, vp, pfc)
    sig("agz_arena_get_forced_playouts", i32, vp, pfc)
    sig("agz_root_select_of", i32, pu32, pf, pf, pu8, i32, i32, C.c_float, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_int))
    sig("agz_pruned_target_of", i32, pi, pu32, pf, pf, i32, i32, i32, C.c_float, C.c_float, C.c_float, pu32, pf)
    ptc = C.POINTER(TargetConf)
    sig("agz_arena_set_policy_target", i32, vp, ptc)
    sig("agz_arena_get_policy_target", i32, vp, ptc)
    sig("agz_visit_target_of", i32, pi, C.POINTER(C.c_uint32), i32, i32, C.c_float, pf)
    sig("agz_arena_begin_move", i32, vp)
    sig("agz_arena_simulate", i32, vp, i32)
    sig("agz_arena_end_move", i32, vp, i32)
    sig("agz_arena_apply_moves", i32, vp, pi)
    sig("agz_arena_get_stats", i32, vp, C.POINTER(ArenaStats))
    sig("agz_arena_get_game", i32, vp, i32, pi, C.POINTER(GameState))
    sig("agz_arena_get_history", i32, vp, i32, pi, i32, pi)
    sig("agz_arena_root_children", i32, vp, i32, i32, pi, pu, pf, pf, i32, pi)
    sig("agz_arena_tree_nodes", i32, vp, i32, i32, pi)
    sig("agz_arena_get_examples", i32, vp, pf, pf, pf, pi, i32, pi)
    sig("agz_arena_clear_examples", i32, vp)
    sig("agz_arena_drop_labelled_examples", i32, vp)
    sig("agz_arena_examples_dev", i32, vp, pvp, pvp, pvp, pi)
    i64, pi64 = C.c_int64, C.POINTER(C.c_int64)
    sig("agz_train_dev", i32, vp, vp, vp, vp, i32, i32, u64, pf)
    sig("agz_examples_create", i32, vp, i32, i32, i32, i32, pvp)
    sig("agz_examples_destroy", None, vp)
    sig("agz_examples_count", i32, vp, pi64)
    sig("agz_examples_clear", i32, vp)
    sig("agz_examples_append_arena", i32, vp, vp)
    sig("agz_examples_append_dev", i32, vp, vp, vp, vp, i64)
    sig("agz_examples_append_host", i32, vp, pf, pf, pf, i64)
    sig("agz_examples_get", i32, vp, pf, pf, pf, i64, pi64)
    sig("agz_examples_augment_rotate", i32, vp)
    sig("agz_examples_prepare", i32, vp, i32, i32, u64, pi)
    sig("agz_examples_tensors_dev", i32, vp, pvp, pvp, pvp, pi64, pi)
    sig("agz_examples_get_tensors", i32, vp, pf, pf, pf)
    sig("agz_examples_raw_dev", i32, vp, pvp, pvp, pvp)
    sig("agz_replay_create", i32, vp, i32, i32, i32, i32, i64, pvp)
    sig("agz_replay_create_packed", i32, vp, i32, i32, i32, i32, i64, pf, i32, pvp)
    sig("agz_encoder_palette", i32, i32, pf, pi)
    sig("agz_replay_pack_host", i32, pf, i64, i32, i32, pf, i32, pu, pi64)
    sig("agz_replay_storage", i32, vp, pi, pi64, pi64)
    sig("agz_replay_destroy", None, vp)
    sig("agz_replay_count", i32, vp, pi64, C.POINTER(C.c_uint64), pi64)
    sig("agz_replay_clear", i32, vp)
    sig("agz_replay_append_examples", i32, vp, vp)
    sig("agz_replay_append_dev", i32, vp, vp, vp, vp, i64)
    sig("agz_replay_append_host", i32, vp, pf, pf, pf, i64)
    sig("agz_replay_get", i32, vp, i64, i64, pf, pf, pf)
    sig("agz_replay_sample_dev", i32, vp, i32, u64, u64, i32, vp, vp, vp)
    sig("agz_replay_sample", i32, vp, i32, u64, u64, i32, pf, pf, pf)
    sig("agz_replay_draw", i32, u64, u64, i32, i64, i32, pi64, pi)
    sig("agz_train_replay", i32, vp, vp, i32, u64, i32, pf)
    sig("agz_replay_sample_slice_dev", i32, vp, i32, i32, i32, u64, u64, i32, vp, vp, vp)
    sig("agz_replay_sample_slice", i32, vp, i32, i32, i32, u64, u64, i32, pf, pf, pf)
    sig("agz_replay_digest", i32, vp, C.POINTER(C.c_uint64))
    sig("agz_replay_digest_host", i32, pf, pf, pf, i64, i32, i32, i32, C.POINTER(C.c_uint64))
    sig("agz_replay_save", i32, vp, C.c_char_p)
    sig("agz_replay_load", i32, vp, C.c_char_p)
    sig("agz_replay_set_ckpt_staging", i32, vp, C.c_size_t)
    sig("agz_train_replay_sharded", i32, vp, vp, i32, u64, i32, i32, pf)
    sig("agz_rotate_boards", i32, vp, pf, i32, i32, i32, pf)
    sig("agz_ctx_prof_set_stride", i32, vp, i32, i32)
    sig("agz_wino_stages", i32, vp, pf, pf, i32, i32, i32, i32, i32, pf, pf)
    sig("agz_wino_h2_tile", i32, i32, i32)
    sig("agz_net_set_wino_h2_form", i32, vp, i32)
    sig("agz_net_set_wino_h2_gemm", i32, vp, i32)
    sig("agz_net_wino_h2_last_rows", i32, vp, C.POINTER(C.c_int), C.POINTER(C.c_int))
    sig("agz_net_last_paths", i32, vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int))
    sig("agz_net_tower_out", i32, vp, i32, pf)
    sig("agz_net_min_same_batch", i32, vp, i32, i32, C.POINTER(C.c_int))
    sig("agz_arena_set_prep_compact", i32, vp, i32)
    sig("agz_arena_set_split", i32, vp, i32)
    sig("agz_arena_split_steps", i32, vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int))
    sig("agz_trainer_set_dma_forward", i32, vp, i32)
    sig("agz_trainer_last_paths", i32, vp, i32, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int))
    sig("agz_trainer_last_rows", i32, vp, i32, C.POINTER(C.c_int32))
    sig("agz_trainer_last_planes", i32, vp, i32, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))
    sig("agz_arena_last_prep_batch", i32, vp, C.POINTER(C.c_int), C.POINTER(C.c_int))
    sig("agz_arena_set_cap_compact", i32, vp, i32)
    sig("agz_arena_last_cap_batch", i32, vp, C.POINTER(C.c_int), C.POINTER(C.c_int))
    sig("agz_arena_debug_counter", i32, vp, i32, C.POINTER(C.c_int64))
    sig("agz_arena_pool_capacity", i32, vp, C.POINTER(C.c_int), C.POINTER(C.c_int))
    sig("agz_wino_h2_chained", i32, i32, i32, i32)
    sig("agz_arena_random_moves", i32, vp, pi, u64)
    sig("agz_arena_set_state", i32, vp, i32, C.POINTER(State))
    sig("agz_arena_save", i32, vp, C.c_char_p)
    sig("agz_arena_load", i32, vp, C.c_char_p)
    sig("agz_arena_set_ckpt_staging", i32, vp, C.c_size_t)
    sig("agz_arena_examples_labelled_dev", i32, vp, pvp)
    sig("agz_mcts_create", i32, vp, C.POINTER(GameConf), C.POINTER(MctsConf), u64, i32, pvp)
    sig("agz_mcts_destroy", None, vp)
    sig("agz_mcts_set_inferencer", i32, vp, i32, vp)
    sig("agz_mcts_set_inferencer_callback", i32, vp, INFER_FN, vp, i32)
    sig("agz_arena_set_inferencer_callback", i32, vp, i32, INFER_FN, vp, i32)
    sig("agz_arena_set_pool_policy", i32, vp, i32)
    sig("agz_mcts_set_pool_policy", i32, vp, i32)
    sig("agz_mcts_set_parallel", i32, vp, i32)
    sig("agz_mcts_set_game", i32, vp, C.POINTER(State))
    sig("agz_mcts_search", i32, vp, i32, pi)
    sig("agz_mcts_policies", i32, vp, pf, i32)
    sig("agz_mcts_root_children", i32, vp, pi, pu, pf, pf, i32, pi)
    sig("agz_mcts_nodes", i32, vp, pi)
    sig("agz_mcts_children", i32, vp, i32, pi, pi, pu, pf, pf, i32, pi)
    sig("agz_mcts_get_stats", i32, vp, C.POINTER(ArenaStats))
    sig("agz_mcts_reset", i32, vp)
    sig("agz_comm_init_all", i32, pvp, i32, pvp)
    sig("agz_comm_unique_id", i32, vp)
    sig("agz_comm_init_rank", i32, vp, i32, i32, vp, pvp)
    sig("agz_comm_destroy", None, vp)
    sig("agz_comm_rank", i32, vp)
    sig("agz_comm_size", i32, vp)
    sig("agz_examples_allgather", i32, vp, vp)
    sig("agz_trainer_allreduce", i32, vp, vp)
    sig("agz_trainer_forward_backward_allreduce", i32, vp, vp, pf, pf, pf, pf)
    sig("agz_trainer_forward_backward_allreduce_dev", i32, vp, vp, vp, vp, vp, pf)
    sig("agz_comm_debug_fail_slice", i32, vp, i32)
    sig("agz_trainer_create_sharded", i32, vp, C.POINTER(NetConf), pvp)
    sig("agz_trainer_create_sharded_tied", i32, vp, C.POINTER(NetConf), pvp)
    sig("agz_trainer_shard", i32, vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32))
    sig("agz_comm_debug_fail_layer", i32, vp, i32)
    _LIB = L
    return L


def _check(r, what=""):
    if r != 0:
        raise AgzError("%s failed (%d): %s" % (what, r, lib().agz_last_error().decode(errors="replace")))


def _pf(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _pi(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


class Ctx:
    def __init__(self, device=0):
        self.h = C.c_void_p()
        self._children = []
        _check(lib().agz_ctx_create(device, C.byref(self.h)), "agz_ctx_create")

    def _adopt(self, child):
        import weakref
        self._children.append(weakref.ref(child))

    def close(self):
        """destroys dependants (arenas, nets) first: their handles hold a pointer to this ctx"""
        if self.h:
            kids = [r() for r in self._children]
            for k in sorted([k for k in kids if k is not None], key=lambda k: 0 if isinstance(k, Arena) else 1):  # arenas first
                k.close()
            self._children = []
            for p in list(getattr(self, "_pinned", {}).values()):
                lib().agz_host_free(self.h, C.c_void_p(p))
            self._pinned = {}
            lib().agz_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def host_array(self, shape, dtype=np.float32):
        """a numpy array over page-locked host memory (agz_host_alloc); freed when the ctx closes or by host_free(array)"""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        _check(lib().agz_host_alloc(self.h, max(n, 1), C.byref(p)), "agz_host_alloc")
        arr = np.ctypeslib.as_array((C.c_char * max(n, 1)).from_address(p.value)).view(dtype)[: int(np.prod(shape))].reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def host_free(self, arr):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p is not None and self.h:
            _check(lib().agz_host_free(self.h, C.c_void_p(p)), "agz_host_free")

    def sync(self):
        _check(lib().agz_ctx_sync(self.h), "agz_ctx_sync")

    def stream(self):
        return lib().agz_ctx_stream(self.h)

    def prof_enable(self, on=True, classes=None):
        """classes: iterable of PROF_* to record (None: all)"""
        if on and classes is not None:
            mask = 0
            for k in classes:
                mask |= 1 << (k + 1)
            _check(lib().agz_ctx_prof_enable(self.h, mask), "agz_ctx_prof_enable")
            return
        return self._prof_enable_all(on)

    def prof_set_stride(self, klass, stride):
        """bracket only every stride-th launch of class klass (agz_debug.h)"""
        _check(lib().agz_ctx_prof_set_stride(self.h, int(klass), int(stride)), "agz_ctx_prof_set_stride")

    def _prof_enable_all(self, on=True):
        _check(lib().agz_ctx_prof_enable(self.h, int(on)), "agz_ctx_prof_enable")

    def prof_read(self, klass):
        n, ms = C.c_int64(0), C.c_double(0)
        _check(lib().agz_ctx_prof_read(self.h, klass, C.byref(n), C.byref(ms)), "agz_ctx_prof_read")
        return n.value, ms.value


class Net:
    """dual.Dual + dual.Inferencer over libagz (dualnet/dual.go, dualnet/meta.go:125-190)."""

    def __init__(self, ctx, K, SharedLayers, FC, Width, Height, Features, ActionSpace, BatchSize=256,
                 bn_mode=BN_DEGENERATE_EPS, bn_eps=1e-5):
        self.ctx = ctx
        self.conf = NetConf(K, SharedLayers, FC, BatchSize, Width, Height, Features, ActionSpace, bn_mode, bn_eps)
        self.h = C.c_void_p()
        _check(lib().agz_net_create(ctx.h, C.byref(self.conf), C.byref(self.h)), "agz_net_create")
        ctx._adopt(self)

    def close(self):
        if self.h and self.ctx.h:
            lib().agz_net_destroy(self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def num_params(self):
        return lib().agz_net_num_params(self.h)

    def param_info(self, i):
        name = C.create_string_buffer(128)
        n = C.c_size_t(0)
        _check(lib().agz_net_param_info(self.h, i, name, 128, C.byref(n)), "agz_net_param_info")
        return name.value.decode(), n.value

    def set_param(self, i, v):
        a = np.ascontiguousarray(v, dtype=np.float32).ravel()
        _check(lib().agz_net_set_param(self.h, i, _pf(a), a.size), "agz_net_set_param")

    def get_param(self, i):
        _, n = self.param_info(i)
        a = np.zeros(n, dtype=np.float32)
        _check(lib().agz_net_get_param(self.h, i, _pf(a), a.size), "agz_net_get_param")
        return a

    def set_bn_stats(self, bi, mean, var):
        m = np.ascontiguousarray(mean, dtype=np.float32)
        v = np.ascontiguousarray(var, dtype=np.float32)
        _check(lib().agz_net_set_bn_stats(self.h, bi, _pf(m), _pf(v), m.size), "agz_net_set_bn_stats")

    def init_random(self, seed):
        _check(lib().agz_net_init_random(self.h, seed), "agz_net_init_random")

    def commit(self):
        _check(lib().agz_net_commit(self.h), "agz_net_commit")

    def infer(self, planes):
        c = self.conf
        x = np.ascontiguousarray(planes, dtype=np.float32).reshape(-1, c.Features, c.Height, c.Width)
        B = x.shape[0]
        pol = np.zeros((B, c.ActionSpace), dtype=np.float32)
        val = np.zeros(B, dtype=np.float32)
        _check(lib().agz_net_infer(self.h, _pf(x), B, _pf(pol), _pf(val)), "agz_net_infer")
        return pol, val

    def set_compute_mode(self, mode):
        _check(lib().agz_net_set_compute_mode(self.h, int(mode)), "agz_net_set_compute_mode")

    def set_latency_mode(self, on=True):
        _check(lib().agz_net_set_latency_mode(self.h, int(on)), "agz_net_set_latency_mode")

    def set_tower_queues(self, queues):
        _check(lib().agz_net_set_tower_queues(self.h, int(queues)), "agz_net_set_tower_queues")

    def set_wino_h2_form(self, form):
        """agz_debug.h A/B hook: -1 auto (chained block where the shape allows), 0 three-kernel block, 1 chained"""
        _check(lib().agz_net_set_wino_h2_form(self.h, int(form)), "agz_net_set_wino_h2_form")

    def set_wino_h2_gemm(self, variant):
        """agz_debug.h A/B hook: 0 default, 1 wino_gemm_h2g_kernel, 2 wino_gemm_h2p_kernel (persistent; K = 256); + 64: round 4's
        store policy; + 128: every transform-domain row kept (no short positions)"""
        _check(lib().agz_net_set_wino_h2_gemm(self.h, int(variant)), "agz_net_set_wino_h2_gemm")

    def wino_h2_last_rows(self):
        """agz_debug.h: (live_r, live_c) of the last chained WINO_H2 block — live rows per 128-row slot at the short positions, 0 = every row kept"""
        r, c = C.c_int(0), C.c_int(0)
        _check(lib().agz_net_wino_h2_last_rows(self.h, C.byref(r), C.byref(c)), "agz_net_wino_h2_last_rows")
        return r.value, c.value

    def last_paths(self):
        """agz_debug.h: (input_conv, block, heads) NPATH_* of the kernels the last whole-batch forward launched"""
        i, b, h = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(lib().agz_net_last_paths(self.h, C.byref(i), C.byref(b), C.byref(h)), "agz_net_last_paths")
        return i.value, b.value, h.value

    def tower_out(self, B):
        """agz_debug.h: the tensor the heads of the last forward of B boards read, [B, K, H, W] float32"""
        c = self.conf
        t = np.zeros((int(B), c.K, c.Height, c.Width), dtype=np.float32)
        _check(lib().agz_net_tower_out(self.h, int(B), _pf(t)), "agz_net_tower_out")
        return t

    def min_same_batch(self, n, G):
        """agz_debug.h: the smallest batch >= n whose per-board outputs equal those of a G-board batch bit for bit"""
        b = C.c_int(0)
        _check(lib().agz_net_min_same_batch(self.h, int(n), int(G), C.byref(b)), "agz_net_min_same_batch")
        return b.value

    def infer_dev(self, planes_ptr, B, policy_ptr, value_ptr):
        """device pointers (ints); asynchronous on the ctx stream"""
        _check(lib().agz_net_infer_dev(self.h, C.c_void_p(planes_ptr), B, C.c_void_p(policy_ptr),
                                       C.c_void_p(value_ptr)), "agz_net_infer_dev")

    def flops_per_eval(self):
        return lib().agz_net_flops_per_eval(self.h)

    def save(self, path):
        _check(lib().agz_net_save(self.h, os.fsencode(path)), "agz_net_save")

    def load(self, path):
        _check(lib().agz_net_load(self.h, os.fsencode(path)), "agz_net_load")


class Trainer:
    """dual.Train on device (dualnet/meta.go:16-54): full-shape learnables, training-mode BN, backward, vanilla SGD."""

    def __init__(self, ctx, K, SharedLayers, FC, Width, Height, Features, ActionSpace, BatchSize, bn_eps=1e-5, tied=False):
        """tied=True (agz_trainer_create_tied): BatchNorm gamma / beta [C,H,W] and FC biases [units] stored once and shared by every batch
        row — the inference net's shapes; their gradient is the sum over the rows"""
        self.ctx = ctx
        self.conf = NetConf(K, SharedLayers, FC, BatchSize, Width, Height, Features, ActionSpace, 0, bn_eps)
        self.h = C.c_void_p()
        if tied:
            _check(lib().agz_trainer_create_tied(ctx.h, C.byref(self.conf), C.byref(self.h)), "agz_trainer_create_tied")
        else:
            _check(lib().agz_trainer_create(ctx.h, C.byref(self.conf), C.byref(self.h)), "agz_trainer_create")
        ctx._adopt(self)

    def is_tied(self):
        """True for a trainer created with tied=True (agz_trainer_is_tied)"""
        v = C.c_int(0)
        _check(lib().agz_trainer_is_tied(self.h, C.byref(v)), "agz_trainer_is_tied")
        return bool(v.value)

    @classmethod
    def sharded(cls, ctx, comm, K, SharedLayers, FC, Width, Height, Features, ActionSpace, BatchSize, bn_eps=1e-5, tied=False):
        """dual.Train at the GLOBAL batch BatchSize split over the ranks of `comm` (agz_trainer_create_sharded): this rank holds rows
        shard() of every batch-shaped learnable; forward_backward / batch / train / train_dev / export / save are collective.
        tied=True (agz_trainer_create_sharded_tied): the tied trainer at the global batch — every rank holds every tied tensor whole, their
        gradients are the ranks' double partials added in rank order, and the replicas step alike"""
        assert comm.ctx is ctx, "the communicator belongs to another context"
        self = cls.__new__(cls)
        self.ctx, self.comm = ctx, comm
        self.conf = NetConf(K, SharedLayers, FC, BatchSize, Width, Height, Features, ActionSpace, 0, bn_eps)
        self.h = C.c_void_p()
        if tied:
            _check(lib().agz_trainer_create_sharded_tied(comm.h, C.byref(self.conf), C.byref(self.h)), "agz_trainer_create_sharded_tied")
        else:
            _check(lib().agz_trainer_create_sharded(comm.h, C.byref(self.conf), C.byref(self.h)), "agz_trainer_create_sharded")
        ctx._adopt(self)
        return self

    def shard(self):
        """(row0, rows, n_ranks): this rank's rows [row0, row0 + rows) of the global batch; a plain trainer: (0, BatchSize, 1)"""
        r0, n, nr = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(lib().agz_trainer_shard(self.h, C.byref(r0), C.byref(n), C.byref(nr)), "agz_trainer_shard")
        return r0.value, n.value, nr.value

    def close(self):
        if self.h and self.ctx.h:
            lib().agz_trainer_destroy(self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def num_params(self):
        return lib().agz_trainer_num_params(self.h)

    def param_info(self, i):
        name = C.create_string_buffer(128)
        n = C.c_size_t(0)
        _check(lib().agz_trainer_param_info(self.h, i, name, 128, C.byref(n)), "agz_trainer_param_info")
        return name.value.decode(), n.value

    def set_param(self, i, v):
        a = np.ascontiguousarray(v, dtype=np.float32).ravel()
        _check(lib().agz_trainer_set_param(self.h, i, _pf(a), a.size), "agz_trainer_set_param")

    def get_param(self, i):
        a = np.zeros(self.param_info(i)[1], np.float32)
        _check(lib().agz_trainer_get_param(self.h, i, _pf(a), a.size), "agz_trainer_get_param")
        return a

    def get_grad(self, i):
        a = np.zeros(self.param_info(i)[1], np.float32)
        _check(lib().agz_trainer_get_grad(self.h, i, _pf(a), a.size), "agz_trainer_get_grad")
        return a

    def init_random(self, seed):
        _check(lib().agz_trainer_init_random(self.h, seed), "agz_trainer_init_random")

    def batch(self, planes, pi, v, lr=0.1):
        x = np.ascontiguousarray(planes, np.float32)
        p = np.ascontiguousarray(pi, np.float32)
        vv = np.ascontiguousarray(v, np.float32)
        c = C.c_float(0)
        _check(lib().agz_trainer_batch(self.h, _pf(x), _pf(p), _pf(vv), lr, C.byref(c)), "agz_trainer_batch")
        return c.value

    def forward_backward(self, planes, pi, v):
        x = np.ascontiguousarray(planes, np.float32)
        p = np.ascontiguousarray(pi, np.float32)
        vv = np.ascontiguousarray(v, np.float32)
        c = C.c_float(0)
        _check(lib().agz_trainer_forward_backward(self.h, _pf(x), _pf(p), _pf(vv), C.byref(c)), "agz_trainer_forward_backward")
        return c.value

    def forward_backward_dev(self, planes_ptr, pi_ptr, v_ptr, want_cost=True):
        c = C.c_float(0)
        _check(lib().agz_trainer_forward_backward_dev(self.h, C.c_void_p(planes_ptr), C.c_void_p(pi_ptr), C.c_void_p(v_ptr),
                                                      C.byref(c) if want_cost else None), "agz_trainer_forward_backward_dev")
        return c.value if want_cost else None

    def apply(self, lr=0.1, grad_scale=1.0):
        _check(lib().agz_trainer_apply(self.h, lr, grad_scale), "agz_trainer_apply")

    def set_solver(self, momentum=0.0, l2reg=0.0, clip=0.0, reserved=0):
        """gorgonia's solver options (agz_trainer_set_solver): L2, then clip, then v = momentum * v - lr * g, w += v; all 0 = vanilla SGD"""
        sc = SolverConf(momentum, l2reg, clip, reserved)
        _check(lib().agz_trainer_set_solver(self.h, C.byref(sc)), "agz_trainer_set_solver")

    def get_solver(self):
        sc = SolverConf()
        _check(lib().agz_trainer_get_solver(self.h, C.byref(sc)), "agz_trainer_get_solver")
        return {"momentum": sc.momentum, "l2reg": sc.l2reg, "clip": sc.clip}

    def get_velocity(self, i):
        """the momentum state of learnable i, shaped and indexed like get_param(i); zeros while the momentum is 0"""
        a = np.zeros(self.param_info(i)[1], np.float32)
        _check(lib().agz_trainer_get_velocity(self.h, i, _pf(a), a.size), "agz_trainer_get_velocity")
        return a

    def set_velocity(self, i, v):
        a = np.ascontiguousarray(v, dtype=np.float32).ravel()
        _check(lib().agz_trainer_set_velocity(self.h, i, _pf(a), a.size), "agz_trainer_set_velocity")

    def reset_solver(self):
        """velocity := 0, the options kept"""
        _check(lib().agz_trainer_reset_solver(self.h), "agz_trainer_reset_solver")

    def set_adam(self, beta1=0.9, beta2=0.999, eps=1e-8, on=True):
        """Adam (agz_trainer_set_adam): L2, then clip, then m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2,
        w -= lr * (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps); excludes a momentum; off releases the moments and resets t"""
        ac = AdamConf(beta1, beta2, eps, int(on))
        _check(lib().agz_trainer_set_adam(self.h, C.byref(ac)), "agz_trainer_set_adam")

    def get_adam(self):
        """the settings in force and the step counter t"""
        ac, t = AdamConf(), C.c_uint64(0)
        _check(lib().agz_trainer_get_adam(self.h, C.byref(ac), C.byref(t)), "agz_trainer_get_adam")
        return {"beta1": ac.beta1, "beta2": ac.beta2, "eps": ac.eps, "on": bool(ac.on), "t": int(t.value)}

    def get_moments(self, i):
        """(m, v) of learnable i, shaped and indexed like get_param(i); zeros while Adam is off"""
        m = np.zeros(self.param_info(i)[1], np.float32)
        v = np.zeros_like(m)
        _check(lib().agz_trainer_get_moments(self.h, i, _pf(m), _pf(v), m.size), "agz_trainer_get_moments")
        return m, v

    def set_moments(self, i, m, v):
        a = np.ascontiguousarray(m, dtype=np.float32).ravel()
        b = np.ascontiguousarray(v, dtype=np.float32).ravel()
        if a.size != b.size:
            raise ValueError("set_moments: m and v differ in size")
        _check(lib().agz_trainer_set_moments(self.h, i, _pf(a), _pf(b), a.size), "agz_trainer_set_moments")

    def set_bn_tracking(self, on=True, momentum=0.997):
        """running BatchNorm statistics (agz_trainer_set_bn_tracking): every training forward adds its batch mean / biased variance to
        accumulators that decay by `momentum`; off keeps the state"""
        _check(lib().agz_trainer_set_bn_tracking(self.h, int(on), momentum), "agz_trainer_set_bn_tracking")

    def get_bn_tracking(self):
        """{"on", "momentum", "weight"}: weight = N, the accumulated weight of the estimates (0: none yet)"""
        on, m, w = C.c_int(0), C.c_float(0), C.c_double(0)
        _check(lib().agz_trainer_get_bn_tracking(self.h, C.byref(on), C.byref(m), C.byref(w)), "agz_trainer_get_bn_tracking")
        return {"on": bool(on.value), "momentum": m.value, "weight": w.value}

    def num_bn(self):
        return lib().agz_trainer_num_bn(self.h)

    def bn_channels(self, bi):
        """channels of BatchNorm op bi (the order of Net.set_bn_stats): K for the tower's ops, 2 / 1 for the policy / value head"""
        n = self.num_bn()
        return self.conf.K if bi < n - 2 else (2 if bi == n - 2 else 1)

    def get_bn_stats(self, bi):
        """(mean, var) estimates of op bi; AGZ_E_STATE while nothing has been tracked"""
        m = np.zeros(self.bn_channels(bi), np.float32)
        v = np.zeros_like(m)
        _check(lib().agz_trainer_get_bn_stats(self.h, bi, _pf(m), _pf(v), m.size), "agz_trainer_get_bn_stats")
        return m, v

    def set_bn_stats(self, bi, mean, var, weight=1.0):
        m = np.ascontiguousarray(mean, np.float32).ravel()
        v = np.ascontiguousarray(var, np.float32).ravel()
        assert m.size == v.size
        _check(lib().agz_trainer_set_bn_stats(self.h, bi, _pf(m), _pf(v), m.size, weight), "agz_trainer_set_bn_stats")

    def reset_bn_stats(self):
        """S = 0, N = 0; the tracking setting is kept"""
        _check(lib().agz_trainer_reset_bn_stats(self.h), "agz_trainer_reset_bn_stats")

    def eval(self, planes, pi, v):
        """the forward pass alone under the tracked statistics (a held-out loss); nothing of the trainer changes"""
        x = np.ascontiguousarray(planes, np.float32)
        p = np.ascontiguousarray(pi, np.float32)
        vv = np.ascontiguousarray(v, np.float32)
        c = C.c_float(0)
        _check(lib().agz_trainer_eval(self.h, _pf(x), _pf(p), _pf(vv), C.byref(c)), "agz_trainer_eval")
        return c.value

    def set_loss(self, kind):
        """the loss kind (agz_trainer_set_loss): LOSS_REFERENCE (default, the reference's cost on raw logits and pre-tanh value) or
        LOSS_ALPHAZERO (softmax cross-entropy and an MSE on tanh); not stored in checkpoints"""
        _check(lib().agz_trainer_set_loss(self.h, int(kind)), "agz_trainer_set_loss")

    def get_loss(self):
        k = C.c_int(0)
        _check(lib().agz_trainer_get_loss(self.h, C.byref(k)), "agz_trainer_get_loss")
        return k.value

    def costs(self):
        """(policy, value): the two terms of the last forward's cost (training or eval)"""
        p, v = C.c_float(0), C.c_float(0)
        _check(lib().agz_trainer_get_costs(self.h, C.byref(p), C.byref(v)), "agz_trainer_get_costs")
        return p.value, v.value

    def eval_dev(self, planes_ptr, pi_ptr, v_ptr, want_cost=True):
        c = C.c_float(0)
        _check(lib().agz_trainer_eval_dev(self.h, C.c_void_p(planes_ptr), C.c_void_p(pi_ptr), C.c_void_p(v_ptr),
                                          C.byref(c) if want_cost else None), "agz_trainer_eval_dev")
        return c.value if want_cost else None

    def set_compute_mode(self, mode):
        _check(lib().agz_trainer_set_compute_mode(self.h, int(mode)), "agz_trainer_set_compute_mode")

    def set_dma_forward(self, on=True):
        """agz_debug.h A/B hook: bit 0 WINO_H2 forward convolutions through the DMA GEMM on pre-split planes (default) or the staging-split
        kernel; bit 2 the first form of the head kernels; bit 3 weight images per layer in line instead of at the start of the step;
        bit 4 no side stream; bit 5 k_conv_h2dma instead of k_conv_h2dma3; bits 6, 7 timing-only decomposition of the latter (wrong results)"""
        _check(lib().agz_trainer_set_dma_forward(self.h, int(on)), "agz_trainer_set_dma_forward")

    def last_paths(self, layer):
        """agz_debug.h test hook: (fwd, wgrad, dgrad, bn_bwd2) — the PATH_* kernels the last step launched for tower layer `layer`"""
        f, w, d, b = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        _check(lib().agz_trainer_last_paths(self.h, int(layer), C.byref(f), C.byref(w), C.byref(d), C.byref(b)), "agz_trainer_last_paths")
        return f.value, w.value, d.value, b.value

    def last_rows(self, layer):
        """agz_debug.h test hook: the eight ROWS_* words of tower layer `layer`'s row plan in the last step (layer SharedLayers + 1: the
        heads, ROWS_HEAD_*), as a tuple"""
        out = (C.c_int32 * 8)()
        _check(lib().agz_trainer_last_rows(self.h, int(layer), out), "agz_trainer_last_rows")
        return tuple(out)

    def last_planes(self, layer):
        """agz_debug.h test hook: (fused, est_bits, range_bits) of tower layer `layer`'s input planes in the last step — written by the
        previous layer's BatchNorm pass and read by the forward; last step's range word (the estimate); this step's range word"""
        f, e, r = C.c_int(0), C.c_uint32(0), C.c_uint32(0)
        _check(lib().agz_trainer_last_planes(self.h, int(layer), C.byref(f), C.byref(e), C.byref(r)), "agz_trainer_last_planes")
        return bool(f.value), e.value, r.value

    def grads_dev(self):
        ptr, n = C.c_void_p(), C.c_size_t(0)
        _check(lib().agz_trainer_grads_dev(self.h, C.byref(ptr), C.byref(n)), "agz_trainer_grads_dev")
        return ptr.value, n.value

    def train(self, Xs, policies, values, batches, iterations, seed=1337):
        """dual.Train; arrays are shuffled in place"""
        assert Xs.dtype == np.float32 and policies.dtype == np.float32 and values.dtype == np.float32
        c = C.c_float(0)
        _check(lib().agz_train(self.h, _pf(Xs), _pf(policies), _pf(values), batches, iterations, seed, C.byref(c)), "agz_train")
        return c.value

    def train_dev(self, Xs_ptr, policies_ptr, values_ptr, batches, iterations, seed=1337):
        """dual.Train over device tensors (see Examples.tensors_dev); nothing is copied to the host"""
        c = C.c_float(0)
        _check(lib().agz_train_dev(self.h, C.c_void_p(Xs_ptr), C.c_void_p(policies_ptr), C.c_void_p(values_ptr), batches,
                                   iterations, seed, C.byref(c)), "agz_train_dev")
        return c.value

    def train_replay(self, replay, steps, seed=1337, symmetric=False):
        """dual.Train's loop over `steps` minibatches sampled from a Replay window (replay_draw(seed, step, BatchSize, len(replay))), each
        sampled straight into the trainer's batch buffers on the device; returns the last step's cost"""
        c = C.c_float(0)
        _check(lib().agz_train_replay(self.h, replay.h if replay is not None else None, int(steps), int(seed) & (2 ** 64 - 1),
                                      1 if symmetric else 0, C.byref(c)), "agz_train_replay")
        return c.value

    def train_replay_sharded(self, replay, steps, seed=1337, symmetric=False, verify=True):
        """train_replay on a sharded handle (agz_train_replay_sharded), COLLECTIVE: every rank calls it with its own replica of the window
        and the same arguments; step s trains on minibatch s of n_ranks * BatchSize rows, this rank on its own rows of it.  The replicas'
        counts are compared at entry, with verify their digests too; a difference raises AgzError on every rank, nothing trained."""
        c = C.c_float(0)
        _check(lib().agz_train_replay_sharded(self.h, replay.h if replay is not None else None, int(steps), int(seed) & (2 ** 64 - 1),
                                              1 if symmetric else 0, 1 if verify else 0, C.byref(c)), "agz_train_replay_sharded")
        return c.value

    def export(self, net):
        _check(lib().agz_trainer_export(self.h, net.h), "agz_trainer_export")

    def save(self, path):
        _check(lib().agz_trainer_save(self.h, str(path).encode()), "agz_trainer_save")

    def load(self, path):
        _check(lib().agz_trainer_load(self.h, str(path).encode()), "agz_trainer_load")


class Arena:
    """n_games x agogo.Arena (arena.go:20-179): batched self-play with per-agent mcts.MCTS trees on device."""

    def __init__(self, ctx, kind, m, n, k=0, komi=0.0, encoder=ENC_TWOPLANE, n_games=1, seed=1337, max_nodes=0,
                 max_moves=0, PUCT=1.0, M=None, N=None, RandomCount=0, Budget=100, RandomMinVisits=0,
                 RandomTemperature=0.0, DumbPass=True, ResignPercentage=0.0, PassPreference=DONT_PREFER_PASS):
        self.ctx = ctx
        self.kind, self.m, self.n, self.n_games = kind, m, n, n_games
        self.features = 18 if encoder == ENC_WQ else 2
        self.action_space = n if kind == GAME_C4 else m * n
        self.gconf = GameConf(kind, m, n, k, komi, max_moves, encoder)
        self.mconf = MctsConf(PUCT, M if M is not None else m, N if N is not None else n, RandomCount, Budget,
                              RandomMinVisits, RandomTemperature, int(DumbPass), ResignPercentage, PassPreference)
        self.h = C.c_void_p()
        self._nets = []
        _check(lib().agz_arena_create(ctx.h, C.byref(self.gconf), C.byref(self.mconf), n_games, seed, max_nodes,
                                      C.byref(self.h)), "agz_arena_create")
        ctx._adopt(self)

    def close(self):
        if self.h and self.ctx.h:
            lib().agz_arena_destroy(self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_inferencer(self, agent, kind, net=None):
        _check(lib().agz_arena_set_inferencer(self.h, agent, kind, net.h if net is not None else None),
               "agz_arena_set_inferencer")
        if net is not None:
            self._nets.append(net)

    def set_inferencer_callback(self, agent, fn, policy_len):
        """AGZ_INF_CALLBACK: agent `agent` evaluates its leaves through the Python function fn(leaves) -> (policy, value) (make_infer_fn)"""
        cfn = make_infer_fn(fn)
        _check(lib().agz_arena_set_inferencer_callback(self.h, agent, cfn, None, int(policy_len)), "agz_arena_set_inferencer_callback")
        self._nets.append(cfn)      # keeps the trampoline alive as long as the arena

    def set_pool_policy(self, policy):
        """POOL_STRICT (a full node pool fails play / selfplay; the default with an explicit max_nodes), POOL_STOP_SEARCH (the reference's
        MAXTREESIZE rule: the search ends early, the game goes on) or POOL_GROW (pools re-allocated before a search could outgrow them; the default
        when the library sized the pools, max_nodes = 0) — include/agz.h"""
        _check(lib().agz_arena_set_pool_policy(self.h, int(policy)), "agz_arena_set_pool_policy")

    def reset(self, a_is_black=None):
        if a_is_black is None:
            _check(lib().agz_arena_reset(self.h, None), "agz_arena_reset")
        else:
            a = np.ascontiguousarray(a_is_black, dtype=np.uint8)
            assert a.size == self.n_games
            _check(lib().agz_arena_reset(self.h, a.ctypes.data_as(C.POINTER(C.c_uint8))), "agz_arena_reset")

    def play(self, n_moves=0, record=True):
        _check(lib().agz_arena_play(self.h, n_moves, int(record)), "agz_arena_play")

    def selfplay(self, n_games_target, record=True):
        _check(lib().agz_arena_selfplay(self.h, n_games_target, int(record)), "agz_arena_selfplay")

    def set_parallel(self, lanes):
        _check(lib().agz_arena_set_parallel(self.h, int(lanes)), "agz_arena_set_parallel")

    def set_leaf_symmetry(self, mode, seed=0):
        """SYM_OFF / SYM_RANDOM / SYM_FIXED + k: leaves of AGZ_INF_NET agents are evaluated under a board symmetry"""
        _check(lib().agz_arena_set_leaf_symmetry(self.h, int(mode), int(seed) & (2 ** 64 - 1)), "agz_arena_set_leaf_symmetry")

    def set_root_noise(self, eps=0.25, alpha=0.3, on=True):
        """Dirichlet noise on the root priors of every search: P = (1 - eps) p + eps eta, eta ~ Dir(alpha) (include/agz.h); default off"""
        conf = NoiseConf(eps, alpha, int(on), 0)
        _check(lib().agz_arena_set_root_noise(self.h, C.byref(conf)), "agz_arena_set_root_noise")

    def get_root_noise(self):
        conf = NoiseConf()
        _check(lib().agz_arena_get_root_noise(self.h, C.byref(conf)), "agz_arena_get_root_noise")
        return {"eps": conf.eps, "alpha": conf.alpha, "on": bool(conf.on)}

    def root_noise(self, g, agent, cap=None):
        """the last draw of `agent`'s tree in game g: (key, moves, eta, n) — n children, min(cap, n) of them copied; n = 0: no draw yet"""
        cap = self.m * self.n + 2 if cap is None else int(cap)
        mv, eta = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float32)
        key, n = C.c_uint64(0), C.c_int(0)
        _check(lib().agz_arena_root_noise(self.h, int(g), int(agent), C.byref(key), _pi(mv), _pf(eta), cap, C.byref(n)), "agz_arena_root_noise")
        k = min(cap, n.value)
        return key.value, mv[:k].copy(), eta[:k].copy(), n.value

    def set_policy_target(self, kind, temperature=1.0):
        """TARGET_REFERENCE (default: the reference's Policies row) or TARGET_VISITS: the policy row of a recorded example is the root's
        visit distribution pi(a) ~ N(a)^(1/temperature), on every searched ply (include/agz.h)"""
        conf = TargetConf(int(kind), temperature, (C.c_int32 * 2)(0, 0))
        _check(lib().agz_arena_set_policy_target(self.h, C.byref(conf)), "agz_arena_set_policy_target")

    def get_policy_target(self):
        conf = TargetConf()
        _check(lib().agz_arena_get_policy_target(self.h, C.byref(conf)), "agz_arena_get_policy_target")
        return {"kind": conf.kind, "temperature": conf.temperature}

    def set_playout_cap(self, p_full=0.25, fast_budget=0, on=True, seed=0, reserved=0):
        """playout cap randomization: every ply of every game is a FULL search (Budget simulations, root noise, a recorded row) with
        probability p_full, else a FAST one (fast_budget simulations, no noise, no row) (include/agz.h); default off"""
        conf = PlayoutCapConf(p_full, int(fast_budget), int(on), int(reserved), int(seed) & (2 ** 64 - 1))
        _check(lib().agz_arena_set_playout_cap(self.h, C.byref(conf)), "agz_arena_set_playout_cap")

    def get_playout_cap(self):
        conf = PlayoutCapConf()
        _check(lib().agz_arena_get_playout_cap(self.h, C.byref(conf)), "agz_arena_get_playout_cap")
        return {"p_full": conf.p_full, "fast_budget": conf.fast_budget, "on": bool(conf.on), "seed": conf.seed}

    def set_forced_playouts(self, k=2.0, on=True, prune=True, reserved=0):
        """forced playouts at the root (a child with n playouts and prior P is selected while n^2 < k P T, T the playouts below the
        root) and, with prune and TARGET_VISITS, the pruned policy target (include/agz.h); default off"""
        conf = ForcedConf(k, int(on), int(prune), int(reserved))
        _check(lib().agz_arena_set_forced_playouts(self.h, C.byref(conf)), "agz_arena_set_forced_playouts")

    def get_forced_playouts(self):
        conf = ForcedConf()
        _check(lib().agz_arena_get_forced_playouts(self.h, C.byref(conf)), "agz_arena_get_forced_playouts")
        return {"k": conf.k, "on": bool(conf.on), "prune": bool(conf.prune)}

    def playout_cap(self, g):
        """the decision of game g's current / last searched ply: (key, ply, kind, budget); kind = -1 before the first one"""
        key, ply, kind, budget = C.c_uint64(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _check(lib().agz_arena_playout_cap(self.h, int(g), C.byref(key), C.byref(ply), C.byref(kind), C.byref(budget)), "agz_arena_playout_cap")
        return key.value, ply.value, kind.value, budget.value

    def playout_cap_counts(self):
        """(plies searched as FULL, as FAST) since the last reset / load"""
        full, fast = C.c_int64(0), C.c_int64(0)
        _check(lib().agz_arena_playout_cap_counts(self.h, C.byref(full), C.byref(fast)), "agz_arena_playout_cap_counts")
        return full.value, fast.value

    def set_cap_compact(self, on=True):
        """agz_debug.h: a playout-cap tail step on the packed batch of the still-searching games (default) or on the whole arena batch"""
        _check(lib().agz_arena_set_cap_compact(self.h, int(on)), "agz_arena_set_cap_compact")

    def last_cap_batch(self):
        """agz_debug.h: (network batch, still-searching games) of the last simulation step if it was a playout-cap tail step, else (0, 0)"""
        b, g = C.c_int(0), C.c_int(0)
        _check(lib().agz_arena_last_cap_batch(self.h, C.byref(b), C.byref(g)), "agz_arena_last_cap_batch")
        return b.value, g.value

    def begin_move(self):
        _check(lib().agz_arena_begin_move(self.h), "agz_arena_begin_move")

    def simulate(self, k):
        _check(lib().agz_arena_simulate(self.h, k), "agz_arena_simulate")

    def end_move(self, record=True):
        _check(lib().agz_arena_end_move(self.h, int(record)), "agz_arena_end_move")

    def apply_moves(self, moves):
        """externally chosen moves (one per game) instead of a search: the opponent's reply in a tournament"""
        m = np.ascontiguousarray(moves, dtype=np.int32)
        assert m.size == self.n_games
        _check(lib().agz_arena_apply_moves(self.h, _pi(m)), "agz_arena_apply_moves")

    def stats(self):
        s = ArenaStats()
        _check(lib().agz_arena_get_stats(self.h, C.byref(s)), "agz_arena_get_stats")
        return {f: getattr(s, f) for f, _ in ArenaStats._fields_}

    def random_moves(self, n_moves, seed=1337):
        """synthetic openings: game g plays n_moves[g] uniformly random legal moves (agz_arena_random_moves)"""
        m = np.ascontiguousarray(n_moves, dtype=np.int32)
        assert m.size == self.n_games
        _check(lib().agz_arena_random_moves(self.h, _pi(m), seed), "agz_arena_random_moves")

    def set_state(self, g, **kw):
        st, keep = make_state(self.m * self.n, **kw)
        _check(lib().agz_arena_set_state(self.h, g, C.byref(st)), "agz_arena_set_state")
        del keep

    def save(self, path):
        """checkpoint of the running arena, between moves (agz_arena_save): games, trees, RNG states, counters, examples"""
        _check(lib().agz_arena_save(self.h, os.fsencode(path)), "agz_arena_save")

    def load(self, path):
        """a checkpoint of an arena of the same game, search configuration and n_games (agz_arena_load); inferencers, lanes and the pool
        policy are the caller's to set again"""
        _check(lib().agz_arena_load(self.h, os.fsencode(path)), "agz_arena_load")

    def set_ckpt_staging(self, nbytes):
        """agz_debug.h: bytes of each staging buffer save / load stream the nodes and examples through"""
        _check(lib().agz_arena_set_ckpt_staging(self.h, int(nbytes)), "agz_arena_set_ckpt_staging")

    def results(self):
        a, b, d = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _check(lib().agz_arena_get_results(self.h, C.byref(a), C.byref(b), C.byref(d)), "agz_arena_get_results")
        return {"a_wins": a.value, "b_wins": b.value, "draws": d.value}

    def game(self, g):
        board = np.zeros(self.m * self.n, dtype=np.int32)
        st = GameState()
        _check(lib().agz_arena_get_game(self.h, g, _pi(board), C.byref(st)), "agz_arena_get_game")
        return board, {f: getattr(st, f) for f, _ in GameState._fields_ if f != "reserved"}

    def history(self, g):
        a = np.zeros(4096, dtype=np.int32)
        n = C.c_int32(0)
        _check(lib().agz_arena_get_history(self.h, g, _pi(a), a.size, C.byref(n)), "agz_arena_get_history")
        return a[:n.value].copy()

    def root_children(self, g, agent):
        cap = self.m * self.n + 2
        mv = np.zeros(cap, dtype=np.int32)
        vis = np.zeros(cap, dtype=np.uint32)
        bs = np.zeros(cap, dtype=np.float32)
        pr = np.zeros(cap, dtype=np.float32)
        n = C.c_int32(0)
        _check(lib().agz_arena_root_children(self.h, g, agent, _pi(mv), vis.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             _pf(bs), _pf(pr), cap, C.byref(n)), "agz_arena_root_children")
        k = n.value
        return mv[:k].copy(), vis[:k].copy(), bs[:k].copy(), pr[:k].copy()

    def set_prep_compact(self, on=True):
        """agz_debug.h: prepareRoot's forward on the packed batch of the roots that need it (default) or on the whole arena batch"""
        _check(lib().agz_arena_set_prep_compact(self.h, int(on)), "agz_arena_set_prep_compact")

    def set_split(self, mode=1):
        """agz_debug.h: 0 = the joined simulation step, 1 = the two half-arenas as pipelines of their own (default where it applies),
        2 = the same with the skew between the halves held by events"""
        _check(lib().agz_arena_set_split(self.h, int(mode)), "agz_arena_set_split")

    def split_steps(self):
        """agz_debug.h: (simulation steps on the split path, on the joined path, whether the last one was split)"""
        s_, j_, l_ = C.c_int64(0), C.c_int64(0), C.c_int(0)
        _check(lib().agz_arena_split_steps(self.h, C.byref(s_), C.byref(j_), C.byref(l_)), "agz_arena_split_steps")
        return s_.value, j_.value, bool(l_.value)

    def last_prep_batch(self):
        """agz_debug.h: (boards the last begin_move's forward ran on, roots it had to evaluate)"""
        b, r = C.c_int(0), C.c_int(0)
        _check(lib().agz_arena_last_prep_batch(self.h, C.byref(b), C.byref(r)), "agz_arena_last_prep_batch")
        return b.value, r.value

    def pool_capacity(self):
        """agz_debug.h: (nodes per pool, re-allocations by POOL_GROW)"""
        c, g = C.c_int(0), C.c_int(0)
        _check(lib().agz_arena_pool_capacity(self.h, C.byref(c), C.byref(g)), "agz_arena_pool_capacity")
        return c.value, g.value

    def max_path_nodes(self):
        """agz_debug.h AGZ_CNT_PATHMAX: nodes on the longest descent since the last reset"""
        v = C.c_int64(0)
        _check(lib().agz_arena_debug_counter(self.h, 15, C.byref(v)), "agz_arena_debug_counter")
        return v.value

    def tree_nodes(self, g, agent):
        n = C.c_int32(0)
        _check(lib().agz_arena_tree_nodes(self.h, g, agent, C.byref(n)), "agz_arena_tree_nodes")
        return n.value

    def examples(self):
        n = C.c_int32(0)
        _check(lib().agz_arena_get_examples(self.h, None, None, None, None, 0, C.byref(n)), "agz_arena_get_examples")
        k = n.value
        cells = self.m * self.n
        planes = np.zeros((k, self.features * cells), np.float32)
        policy = np.zeros((k, self.action_space + 1), np.float32)
        value = np.zeros(k, np.float32)
        gidx = np.zeros(k, np.int32)
        if k:
            _check(lib().agz_arena_get_examples(self.h, _pf(planes), _pf(policy), _pf(value), _pi(gidx), k,
                                                C.byref(n)), "agz_arena_get_examples")
        return planes, policy, value, gidx

    def clear_examples(self):
        _check(lib().agz_arena_clear_examples(self.h), "agz_arena_clear_examples")


def make_state(cells, board, to_move, n_moves=0, passes=0, hash=0, captures=(0.0, 0.0), last_moves=(), historical=()):
    """agz_state from numpy pieces; returns (struct, keep-alive list)"""
    b = np.ascontiguousarray(board, dtype=np.int32).reshape(-1)
    assert b.size == cells
    lm = np.ascontiguousarray(last_moves, dtype=np.int32).reshape(-1)
    hs = np.ascontiguousarray(historical, dtype=np.int32).reshape(-1)
    assert hs.size % cells == 0
    st = State()
    st.board = _pi(b)
    st.to_move, st.n_moves, st.passes, st.hash = int(to_move), int(n_moves), int(passes), int(hash) & 0xFFFFFFFF
    st.captures_black, st.captures_white = float(captures[0]), float(captures[1])
    st.last_moves = _pi(lm) if lm.size else None
    st.n_last_moves = lm.size
    st.historical = _pi(hs) if hs.size else None
    st.n_historical = hs.size // cells
    return st, [b, lm, hs]


class Mcts:
    """mcts.MCTS (mcts/tree.go:80-142, search.go:92): one search tree on a caller-owned game.State."""

    def __init__(self, ctx, kind, m, n, k=0, komi=0.0, encoder=ENC_TWOPLANE, seed=1337, max_nodes=0, max_moves=0, PUCT=1.0,
                 M=None, N=None, RandomCount=0, Budget=100, RandomMinVisits=0, RandomTemperature=0.0, DumbPass=True,
                 ResignPercentage=0.0, PassPreference=DONT_PREFER_PASS):
        self.ctx = ctx
        self.kind, self.m, self.n = kind, m, n
        self.action_space = n if kind == GAME_C4 else m * n
        self.gconf = GameConf(kind, m, n, k, komi, max_moves, encoder)
        self.mconf = MctsConf(PUCT, M if M is not None else m, N if N is not None else n, RandomCount, Budget,
                              RandomMinVisits, RandomTemperature, int(DumbPass), ResignPercentage, PassPreference)
        self.h = C.c_void_p()
        self._nets = []
        _check(lib().agz_mcts_create(ctx.h, C.byref(self.gconf), C.byref(self.mconf), seed, max_nodes, C.byref(self.h)),
               "agz_mcts_create")
        ctx._adopt(self)

    def close(self):
        if self.h and self.ctx.h:
            lib().agz_mcts_destroy(self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_inferencer(self, kind, net=None):
        _check(lib().agz_mcts_set_inferencer(self.h, kind, net.h if net is not None else None), "agz_mcts_set_inferencer")
        if net is not None:
            self._nets.append(net)

    def set_inferencer_callback(self, fn, policy_len):
        """mcts.New(game, conf, nn) with a caller-supplied Inferencer: fn(leaves) -> (policy, value) (make_infer_fn)"""
        cfn = make_infer_fn(fn)
        _check(lib().agz_mcts_set_inferencer_callback(self.h, cfn, None, int(policy_len)), "agz_mcts_set_inferencer_callback")
        self._nets.append(cfn)

    def set_pool_policy(self, policy):
        _check(lib().agz_mcts_set_pool_policy(self.h, int(policy)), "agz_mcts_set_pool_policy")

    def set_parallel(self, lanes):
        _check(lib().agz_mcts_set_parallel(self.h, int(lanes)), "agz_mcts_set_parallel")

    def set_leaf_symmetry(self, mode, seed=0):
        _check(lib().agz_mcts_set_leaf_symmetry(self.h, int(mode), int(seed) & (2 ** 64 - 1)), "agz_mcts_set_leaf_symmetry")

    def set_root_noise(self, eps=0.25, alpha=0.3, on=True):
        conf = NoiseConf(eps, alpha, int(on), 0)
        _check(lib().agz_mcts_set_root_noise(self.h, C.byref(conf)), "agz_mcts_set_root_noise")

    def root_noise(self, cap=None):
        """the tree's last draw: (key, moves, eta, n), as Arena.root_noise"""
        cap = self.m * self.n + 2 if cap is None else int(cap)
        mv, eta = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float32)
        key, n = C.c_uint64(0), C.c_int(0)
        _check(lib().agz_mcts_root_noise(self.h, C.byref(key), _pi(mv), _pf(eta), cap, C.byref(n)), "agz_mcts_root_noise")
        k = min(cap, n.value)
        return key.value, mv[:k].copy(), eta[:k].copy(), n.value

    def set_game(self, **kw):
        st, keep = make_state(self.m * self.n, **kw)
        _check(lib().agz_mcts_set_game(self.h, C.byref(st)), "agz_mcts_set_game")
        del keep

    def search(self, player):
        best = C.c_int32(0)
        _check(lib().agz_mcts_search(self.h, int(player), C.byref(best)), "agz_mcts_search")
        return best.value

    def policies(self):
        p = np.zeros(self.action_space + 1, np.float32)
        _check(lib().agz_mcts_policies(self.h, _pf(p), p.size), "agz_mcts_policies")
        return p

    def root_children(self):
        cap = self.m * self.n + 2
        mv = np.zeros(cap, dtype=np.int32)
        vis = np.zeros(cap, dtype=np.uint32)
        bs = np.zeros(cap, dtype=np.float32)
        pr = np.zeros(cap, dtype=np.float32)
        n = C.c_int32(0)
        _check(lib().agz_mcts_root_children(self.h, _pi(mv), vis.ctypes.data_as(C.POINTER(C.c_uint32)), _pf(bs), _pf(pr), cap,
                                            C.byref(n)), "agz_mcts_root_children")
        k = n.value
        return mv[:k].copy(), vis[:k].copy(), bs[:k].copy(), pr[:k].copy()

    def nodes(self):
        n = C.c_int32(0)
        _check(lib().agz_mcts_nodes(self.h, C.byref(n)), "agz_mcts_nodes")
        return n.value

    def set_timeout_ms(self, ms):
        """mcts.Config.Timeout (tree.go:18): > 0 = search by wall clock (not deterministic); 0 = exactly Budget simulations"""
        _check(lib().agz_mcts_set_timeout_ms(self.h, int(ms)), "agz_mcts_set_timeout_ms")

    def last_simulations(self):
        n = C.c_int64(0)
        _check(lib().agz_mcts_last_simulations(self.h, C.byref(n)), "agz_mcts_last_simulations")
        return n.value

    def to_dot(self, max_nodes=0):
        """(*MCTS).ToDot (mcts/graph.go:34): Graphviz text of the live tree.  max_nodes = 0 (default, as the reference and the Go shim):
        the whole tree — hundreds of MB for a deep 19x19 tree; max_nodes > 0: the first max_nodes nodes (a top of the tree)"""
        need = C.c_size_t(0)
        _check(lib().agz_mcts_to_dot(self.h, int(max_nodes), None, 0, C.byref(need)), "agz_mcts_to_dot")
        buf = C.create_string_buffer(need.value)
        _check(lib().agz_mcts_to_dot(self.h, int(max_nodes), buf, need.value, C.byref(need)), "agz_mcts_to_dot")
        return buf.value.decode("utf-8")

    def children(self, node=0):
        """(*MCTS).Children(of): ids, moves, visits, blackScores, priors of the children of any node (0 = root)"""
        cap = self.m * self.n + 2
        ids = np.zeros(cap, dtype=np.int32)
        mv = np.zeros(cap, dtype=np.int32)
        vis = np.zeros(cap, dtype=np.uint32)
        bs = np.zeros(cap, dtype=np.float32)
        pr = np.zeros(cap, dtype=np.float32)
        n = C.c_int32(0)
        _check(lib().agz_mcts_children(self.h, int(node), _pi(ids), _pi(mv), vis.ctypes.data_as(C.POINTER(C.c_uint32)), _pf(bs),
                                       _pf(pr), cap, C.byref(n)), "agz_mcts_children")
        k = n.value
        return ids[:k].copy(), mv[:k].copy(), vis[:k].copy(), bs[:k].copy(), pr[:k].copy()

    def stats(self):
        s = ArenaStats()
        _check(lib().agz_mcts_get_stats(self.h, C.byref(s)), "agz_mcts_get_stats")
        return {f: getattr(s, f) for f, _ in ArenaStats._fields_}

    def reset(self):
        _check(lib().agz_mcts_reset(self.h), "agz_mcts_reset")


class Comm:
    """agz_comm: an RCCL communicator over the devices of agz_ctx handles."""

    def __init__(self, h, ctx):
        self.h, self.ctx = h, ctx
        ctx._adopt(self)

    @staticmethod
    def init_all(ctxs):
        n = len(ctxs)
        arr = (C.c_void_p * n)(*[c.h for c in ctxs])
        out = (C.c_void_p * n)()
        _check(lib().agz_comm_init_all(arr, n, out), "agz_comm_init_all")
        return [Comm(C.c_void_p(out[i]), ctxs[i]) for i in range(n)]

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        _check(lib().agz_comm_unique_id(buf), "agz_comm_unique_id")
        return buf.raw

    @staticmethod
    def init_rank(ctx, n_ranks, rank, id_bytes):
        out = C.c_void_p()
        buf = C.create_string_buffer(bytes(id_bytes), 128)
        _check(lib().agz_comm_init_rank(ctx.h, n_ranks, rank, buf, C.byref(out)), "agz_comm_init_rank")
        return Comm(out, ctx)

    def close(self):
        if self.h and self.ctx.h:
            lib().agz_comm_destroy(self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rank(self):
        return lib().agz_comm_rank(self.h)

    def size(self):
        return lib().agz_comm_size(self.h)

    def allgather_examples(self, ex):
        _check(lib().agz_examples_allgather(self.h, ex.h), "agz_examples_allgather")

    def allreduce_trainer(self, trainer):
        _check(lib().agz_trainer_allreduce(self.h, trainer.h), "agz_trainer_allreduce")

    def forward_backward_allreduce(self, trainer, planes, pi, v):
        """the data-parallel step's gradients: forward / backward on this rank's batch with every slice of the flat gradient buffer
        summed over the ranks while the rest of the backward runs (agz_trainer_forward_backward_allreduce)"""
        x = np.ascontiguousarray(planes, np.float32)
        p = np.ascontiguousarray(pi, np.float32)
        vv = np.ascontiguousarray(v, np.float32)
        c = C.c_float(0)
        _check(lib().agz_trainer_forward_backward_allreduce(self.h, trainer.h, _pf(x), _pf(p), _pf(vv), C.byref(c)),
               "agz_trainer_forward_backward_allreduce")
        return c.value

    def debug_fail_slice(self, k):
        """agz_debug.h: this rank's next data-parallel step fails right before slice k (failure injection for the N > 1 tests)"""
        _check(lib().agz_comm_debug_fail_slice(self.h, int(k)), "agz_comm_debug_fail_slice")

    def debug_fail_layer(self, layer):
        """agz_debug.h: this rank's next sharded-trainer step fails right before layer `layer`'s first exchange (L + 1: the heads)"""
        _check(lib().agz_comm_debug_fail_layer(self.h, int(layer)), "agz_comm_debug_fail_layer")

    def forward_backward_allreduce_dev(self, trainer, planes_ptr, pi_ptr, v_ptr, want_cost=True):
        c = C.c_float(0)
        _check(lib().agz_trainer_forward_backward_allreduce_dev(self.h, trainer.h, C.c_void_p(planes_ptr), C.c_void_p(pi_ptr), C.c_void_p(v_ptr),
                                                                C.byref(c) if want_cost else None), "agz_trainer_forward_backward_allreduce_dev")
        return c.value if want_cost else None


class Examples:
    """[]agogo.Example on device + Augmenter / shuffleExamples / prepareExamples (agogo.go:110-133, 211-257)."""

    def __init__(self, ctx, Features, Height, Width, PolicyLen):
        self.ctx = ctx
        self.F, self.H, self.W, self.A1 = Features, Height, Width, PolicyLen
        self.h = C.c_void_p()
        _check(lib().agz_examples_create(ctx.h, Features, Height, Width, PolicyLen, C.byref(self.h)), "agz_examples_create")
        ctx._adopt(self)

    def close(self):
        if self.h and self.ctx.h:
            lib().agz_examples_destroy(self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        n = C.c_int64(0)
        _check(lib().agz_examples_count(self.h, C.byref(n)), "agz_examples_count")
        return n.value

    def clear(self):
        _check(lib().agz_examples_clear(self.h), "agz_examples_clear")

    def append_arena(self, arena):
        _check(lib().agz_examples_append_arena(self.h, arena.h), "agz_examples_append_arena")

    def append_dev(self, planes_ptr, policy_ptr, value_ptr, n):
        _check(lib().agz_examples_append_dev(self.h, C.c_void_p(planes_ptr), C.c_void_p(policy_ptr), C.c_void_p(value_ptr), n),
               "agz_examples_append_dev")

    def append_host(self, planes, policy, value):
        p = np.ascontiguousarray(planes, np.float32)
        q = np.ascontiguousarray(policy, np.float32)
        v = np.ascontiguousarray(value, np.float32)
        n = v.size
        assert p.size == n * self.F * self.H * self.W and q.size == n * self.A1
        _check(lib().agz_examples_append_host(self.h, _pf(p), _pf(q), _pf(v), n), "agz_examples_append_host")

    def get(self):
        n = len(self)
        p = np.zeros((n, self.F * self.H * self.W), np.float32)
        q = np.zeros((n, self.A1), np.float32)
        v = np.zeros(n, np.float32)
        k = C.c_int64(0)
        _check(lib().agz_examples_get(self.h, _pf(p), _pf(q), _pf(v), n, C.byref(k)), "agz_examples_get")
        return p, q, v

    def raw_dev(self):
        """device pointers of the raw store (Board, Policy, Value rows in append order)"""
        x, p, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().agz_examples_raw_dev(self.h, C.byref(x), C.byref(p), C.byref(v)), "agz_examples_raw_dev")
        return x.value, p.value, v.value

    def augment_rotate(self):
        _check(lib().agz_examples_augment_rotate(self.h), "agz_examples_augment_rotate")

    def augment_dihedral(self):
        """every example e -> [S_0 e .. S_7 e] (the eight board symmetries, symmetry_map)"""
        _check(lib().agz_examples_augment_dihedral(self.h), "agz_examples_augment_dihedral")

    def prepare(self, BatchSize, maxExamples=0, seed=1337):
        b = C.c_int32(0)
        _check(lib().agz_examples_prepare(self.h, BatchSize, maxExamples, seed, C.byref(b)), "agz_examples_prepare")
        return b.value

    def tensors_dev(self):
        x, p, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
        rows, b = C.c_int64(0), C.c_int32(0)
        _check(lib().agz_examples_tensors_dev(self.h, C.byref(x), C.byref(p), C.byref(v), C.byref(rows), C.byref(b)),
               "agz_examples_tensors_dev")
        return x.value, p.value, v.value, rows.value, b.value

    def tensors(self):
        _, _, _, rows, _ = self.tensors_dev()
        x = np.zeros((rows, self.F, self.H, self.W), np.float32)
        p = np.zeros((rows, self.A1), np.float32)
        v = np.zeros(rows, np.float32)
        _check(lib().agz_examples_get_tensors(self.h, _pf(x), _pf(p), _pf(v)), "agz_examples_get_tensors")
        return x, p, v


class Replay:
    """A sliding window over the most recent `capacity` examples on the device, and its sampler: minibatches drawn uniformly with
    replacement, each row under a random board symmetry applied as it is drawn (agz_replay, include/agz.h).  Logical row 0 is the oldest.
    With a `palette` (1 to 4 float32 values taken as bit patterns, e.g. encoder_palette(enc)) the planes are kept as 2-bit codes
    (agz_replay_create_packed): appends then take all rows or none, a cell outside the palette raises AgzError."""

    def __init__(self, ctx, Features, Height, Width, PolicyLen, capacity, palette=None):
        self.ctx = ctx
        self.F, self.H, self.W, self.A1 = Features, Height, Width, PolicyLen
        self.h = C.c_void_p()
        if palette is None:
            _check(lib().agz_replay_create(ctx.h, Features, Height, Width, PolicyLen, int(capacity), C.byref(self.h)), "agz_replay_create")
        else:
            pal = np.ascontiguousarray(palette, np.float32).ravel()
            _check(lib().agz_replay_create_packed(ctx.h, Features, Height, Width, PolicyLen, int(capacity), _pf(pal), int(pal.size),
                                                  C.byref(self.h)), "agz_replay_create_packed")
        ctx._adopt(self)

    def storage(self):
        """(packed, row_bytes, device_bytes): the kind of the window, the bytes of one stored row and of the whole ring on the device"""
        packed, row, dev = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        _check(lib().agz_replay_storage(self.h, C.byref(packed), C.byref(row), C.byref(dev)), "agz_replay_storage")
        return bool(packed.value), row.value, dev.value

    def close(self):
        if self.h and self.ctx.h:
            lib().agz_replay_destroy(self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _count(self):
        live, total, cap = C.c_int64(0), C.c_uint64(0), C.c_int64(0)
        _check(lib().agz_replay_count(self.h, C.byref(live), C.byref(total), C.byref(cap)), "agz_replay_count")
        return live.value, total.value, cap.value

    def __len__(self):
        """live rows: min(total, capacity)"""
        return self._count()[0]

    def total(self):
        """rows ever appended"""
        return self._count()[1]

    @property
    def capacity(self):
        return self._count()[2]

    def clear(self):
        _check(lib().agz_replay_clear(self.h), "agz_replay_clear")

    def append_examples(self, ex):
        """the raw store of an Examples set, in append order, device to device; `ex` is unchanged"""
        _check(lib().agz_replay_append_examples(self.h, ex.h), "agz_replay_append_examples")

    def append_dev(self, planes_ptr, policy_ptr, value_ptr, n):
        _check(lib().agz_replay_append_dev(self.h, C.c_void_p(planes_ptr), C.c_void_p(policy_ptr), C.c_void_p(value_ptr), n),
               "agz_replay_append_dev")

    def append_host(self, planes, policy, value):
        p = np.ascontiguousarray(planes, np.float32)
        q = np.ascontiguousarray(policy, np.float32)
        v = np.ascontiguousarray(value, np.float32)
        n = v.size
        assert p.size == n * self.F * self.H * self.W and q.size == n * self.A1
        _check(lib().agz_replay_append_host(self.h, _pf(p), _pf(q), _pf(v), n), "agz_replay_append_host")

    def get(self, j0=0, cnt=None):
        """logical rows [j0, j0 + cnt), oldest first (default: every live row)"""
        if cnt is None:
            cnt = len(self) - j0
        p = np.zeros((max(cnt, 0), self.F * self.H * self.W), np.float32)
        q = np.zeros((max(cnt, 0), self.A1), np.float32)
        v = np.zeros(max(cnt, 0), np.float32)
        _check(lib().agz_replay_get(self.h, int(j0), int(cnt), _pf(p), _pf(q), _pf(v)), "agz_replay_get")
        return p, q, v

    def sample(self, rows, seed, step=0, symmetric=False):
        """minibatch `step` on the host: X [rows, F, H, W], Pi [rows, PolicyLen], V [rows]"""
        x = np.zeros((max(rows, 1), self.F, self.H, self.W), np.float32)
        p = np.zeros((max(rows, 1), self.A1), np.float32)
        v = np.zeros(max(rows, 1), np.float32)
        _check(lib().agz_replay_sample(self.h, int(rows), int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), 1 if symmetric else 0,
                                       _pf(x), _pf(p), _pf(v)), "agz_replay_sample")
        return x, p, v

    def sample_dev(self, rows, seed, step, symmetric, X_ptr, Pi_ptr, V_ptr):
        """minibatch `step` into device buffers, asynchronous on the context's queue"""
        _check(lib().agz_replay_sample_dev(self.h, int(rows), int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), 1 if symmetric else 0,
                                           C.c_void_p(X_ptr), C.c_void_p(Pi_ptr), C.c_void_p(V_ptr)), "agz_replay_sample_dev")

    def sample_slice(self, rows, row0, cnt, seed, step=0, symmetric=False):
        """rows [row0, row0 + cnt) of minibatch `step` of `rows` rows on the host: X [cnt, F, H, W], Pi [cnt, PolicyLen], V [cnt]"""
        x = np.zeros((max(cnt, 1), self.F, self.H, self.W), np.float32)
        p = np.zeros((max(cnt, 1), self.A1), np.float32)
        v = np.zeros(max(cnt, 1), np.float32)
        _check(lib().agz_replay_sample_slice(self.h, int(rows), int(row0), int(cnt), int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1),
                                             1 if symmetric else 0, _pf(x), _pf(p), _pf(v)), "agz_replay_sample_slice")
        return x, p, v

    def sample_slice_dev(self, rows, row0, cnt, seed, step, symmetric, X_ptr, Pi_ptr, V_ptr):
        """the same slice into device buffers of cnt rows, asynchronous on the context's queue"""
        _check(lib().agz_replay_sample_slice_dev(self.h, int(rows), int(row0), int(cnt), int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1),
                                                 1 if symmetric else 0, C.c_void_p(X_ptr), C.c_void_p(Pi_ptr), C.c_void_p(V_ptr)),
               "agz_replay_sample_slice_dev")

    def digest(self):
        """the uint64 digest of the window's logical content, computed on the device (agz_replay_digest): equal for replicas holding the
        same rows in the same order, packed or not, wherever their rings sit"""
        d = C.c_uint64(0)
        _check(lib().agz_replay_digest(self.h, C.byref(d)), "agz_replay_digest")
        return d.value

    def save(self, path):
        """checkpoint of the window (agz_replay_save): the live rows in logical order, total, form and digest; `path` is replaced only
        once the file is complete"""
        _check(lib().agz_replay_save(self.h, os.fsencode(path)), "agz_replay_save")

    def load(self, path):
        """replace the window's content by a checkpoint of a window of the same row shape (agz_replay_load); capacity and form may
        differ.  The whole file is validated first: after an AgzError the window is as it was"""
        _check(lib().agz_replay_load(self.h, os.fsencode(path)), "agz_replay_load")

    def set_ckpt_staging(self, nbytes):
        """tests: the size of the staging buffers save / load stream through (agz_debug.h)"""
        _check(lib().agz_replay_set_ckpt_staging(self.h, int(nbytes)), "agz_replay_set_ckpt_staging")


def replay_digest_host(planes, policy, value, Features, cells, PolicyLen):
    """the digest of n rows in host arrays, in logical order (replay.hpp through agz_replay_digest_host; host only):
    replay_digest_host(*rp.get(), F, H * W, A1) == rp.digest()"""
    p = np.ascontiguousarray(planes, np.float32)
    q = np.ascontiguousarray(policy, np.float32)
    v = np.ascontiguousarray(value, np.float32)
    n = v.size
    assert p.size == n * Features * cells and q.size == n * PolicyLen
    d = C.c_uint64(0)
    _check(lib().agz_replay_digest_host(_pf(p), _pf(q), _pf(v), n, int(Features), int(cells), int(PolicyLen), C.byref(d)),
           "agz_replay_digest_host")
    return d.value


def replay_draw(seed, step, rows, n, symmetric=True):
    """(j [rows], k [rows]) of minibatch `step` over n live rows (replay.hpp; host only): the rows and symmetries Replay.sample draws"""
    j = np.zeros(max(int(rows), 1), np.int64)
    k = np.zeros(max(int(rows), 1), np.int32)
    _check(lib().agz_replay_draw(int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), int(rows), int(n), 1 if symmetric else 0,
                                 j.ctypes.data_as(C.POINTER(C.c_int64)), _pi(k)), "agz_replay_draw")
    return j[:int(rows)], k[:int(rows)]


def encoder_palette(encoder):
    """the bit patterns an encoder's planes hold, as float32 (agz_encoder_palette; host only): a packed Replay's palette"""
    pal = np.zeros(4, np.float32)
    n = C.c_int32(0)
    _check(lib().agz_encoder_palette(int(encoder), _pf(pal), C.byref(n)), "agz_encoder_palette")
    return pal[:n.value]


def replay_pack_host(planes, Features, cells, palette, validate_only=False):
    """(words [n, Features * ((cells + 15) // 16)] uint32 or None, first_bad) of n rows of planes under a palette (replay_pack.hpp through
    agz_replay_pack_host; host only).  first_bad is -1, or the smallest linear element index outside the palette; words is then None."""
    p = np.ascontiguousarray(planes, np.float32)
    pal = np.ascontiguousarray(palette, np.float32).ravel()
    n = p.size // (Features * cells)
    assert p.size == n * Features * cells
    words = None if validate_only else np.zeros((n, Features * ((cells + 15) // 16)), np.uint32)
    bad = C.c_int64(-1)
    r = lib().agz_replay_pack_host(_pf(p), n, int(Features), int(cells), _pf(pal), int(pal.size),
                                   None if words is None else words.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(bad))
    if r != 0 and bad.value < 0:
        _check(r, "agz_replay_pack_host")
    return (words if r == 0 else None), bad.value


def wino_h2_chained(H, W, K):
    """agz_debug.h: 1 when AGZ_COMPUTE_WINO_H2 takes the chained block on this shape"""
    return int(lib().agz_wino_h2_chained(H, W, K))


def wino_h2_tile(H, W):
    """measurement: Winograd tile size (4 or 5) COMPUTE_WINO_H2 uses on an H x W board (agz_debug.h)"""
    return int(lib().agz_wino_h2_tile(H, W))


def wino_stages(ctx, x, w):
    """diagnostics: Winograd F(4x4,3x3) input transform and transform-domain GEMMs. x [B,H,W,C], w [N,C,3,3] -> V [36,T,C], M [36,T,N]"""
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    B, H, W, Cc = x.shape
    N = w.shape[0]
    T = B * ((H + 3) // 4) * ((W + 3) // 4)
    V = np.zeros((36, T, Cc), np.float32)
    M = np.zeros((36, T, N), np.float32)
    _check(lib().agz_wino_stages(ctx.h, _pf(x), _pf(w), B, H, W, Cc, N, _pf(V), _pf(M)), "agz_wino_stages")
    return V, M


def rotate_boards(ctx, boards, m, n):
    """RotateBoard (encoding_helper.go:80-107) on a stack of m x n boards"""
    b = np.ascontiguousarray(boards, np.float32)
    count = b.size // (m * n)
    out = np.zeros_like(b)
    _check(lib().agz_rotate_boards(ctx.h, _pf(b), count, m, n, _pf(out)), "agz_rotate_boards")
    return out


def symmetry_boards(ctx, boards, m, k):
    """S_k (symmetry_map) on a stack of m x m boards, on the device"""
    b = np.ascontiguousarray(boards, np.float32)
    count = b.size // (m * m)
    out = np.zeros_like(b)
    _check(lib().agz_symmetry_boards(ctx.h, _pf(b), count, m, int(k), _pf(out)), "agz_symmetry_boards")
    return out


def symmetry_map(m, k):
    """src_k: (S_k x).flat[c] == x.flat[src[c]] for an m x m board x (host only)"""
    src = np.zeros(m * m, np.int32)
    _check(lib().agz_symmetry_map(int(m), int(k), _pi(src)), "agz_symmetry_map")
    return src


def symmetry_inverse(k):
    """inv(k): S_inv(k) o S_k = id (host only)"""
    r = lib().agz_symmetry_inverse(int(k))
    _check(min(r, 0), "agz_symmetry_inverse")
    return r


def leaf_symmetry_of(seed, board, to_move):
    """SYM_RANDOM's k for a position: board = cells of NONE / BLACK / WHITE, row-major (host only)"""
    b = np.ascontiguousarray(board, np.int32).reshape(-1)
    k = C.c_int(0)
    _check(lib().agz_leaf_symmetry_of(int(seed) & (2 ** 64 - 1), _pi(b), b.size, int(to_move), C.byref(k)), "agz_leaf_symmetry_of")
    return k.value


def root_noise_of(key, n, alpha):
    """eta[0..n) of the root-noise draw `key` (noise.hpp; host only): what the device mixes into n root children"""
    eta = np.zeros(max(int(n), 1), np.float32)
    _check(lib().agz_root_noise_of(int(key) & (2 ** 64 - 1), int(n), float(alpha), _pf(eta)), "agz_root_noise_of")
    return eta[:int(n)]


def playout_cap_of(seed, key, ply, p_full):
    """CAP_FULL / CAP_FAST of ply `ply` of the game slot with key `key` under the playout cap (cap.hpp; host only)"""
    kind = C.c_int32(0)
    _check(lib().agz_playout_cap_of(int(seed) & (2 ** 64 - 1), int(key) & (2 ** 64 - 1), int(ply), p_full, C.byref(kind)), "agz_playout_cap_of")
    return kind.value


def root_select_of(visits, black_scores, priors, player, puct, k, marks=None):
    """(block index, forced) of Node.Select at a root with the forced-playout rule (forced.hpp; host only): the child the device
    descends to from a root whose read-back is (visits, black_scores, priors); marks = the children's virtual-loss marks in a lane
    round, None in the sequential search; k = 0 is plain Node.Select"""
    vis = np.ascontiguousarray(visits, dtype=np.uint32).reshape(-1)
    bs = np.ascontiguousarray(black_scores, dtype=np.float32).reshape(-1)
    pr = np.ascontiguousarray(priors, dtype=np.float32).reshape(-1)
    assert vis.size == bs.size == pr.size
    mk = None if marks is None else np.ascontiguousarray(marks, dtype=np.uint8).reshape(-1)
    assert mk is None or mk.size == vis.size
    idx, forced = C.c_int(0), C.c_int(0)
    _check(lib().agz_root_select_of(vis.ctypes.data_as(C.POINTER(C.c_uint32)), _pf(bs), _pf(pr),
                                    None if mk is None else mk.ctypes.data_as(C.POINTER(C.c_uint8)), vis.size, int(player), puct, k,
                                    C.byref(idx), C.byref(forced)), "agz_root_select_of")
    return idx.value, bool(forced.value)


def pruned_target_of(moves, visits, black_scores, priors, action_space, player, puct, k, temperature=1.0):
    """(row, pruned playouts) of a root under forced playouts with pruning (forced.hpp; host only): the policy row (action_space + 1
    floats, Pass last) the device records for a root whose read-back is (moves, visits, black_scores, priors), and n'_i per child"""
    mv = np.ascontiguousarray(moves, dtype=np.int32).reshape(-1)
    vis = np.ascontiguousarray(visits, dtype=np.uint32).reshape(-1)
    bs = np.ascontiguousarray(black_scores, dtype=np.float32).reshape(-1)
    pr = np.ascontiguousarray(priors, dtype=np.float32).reshape(-1)
    assert mv.size == vis.size == bs.size == pr.size
    row = np.zeros(max(int(action_space), 0) + 1, np.float32)
    npl = np.zeros(max(mv.size, 1), np.uint32)
    _check(lib().agz_pruned_target_of(_pi(mv), vis.ctypes.data_as(C.POINTER(C.c_uint32)), _pf(bs), _pf(pr), mv.size, int(action_space), int(player),
                                      puct, k, temperature, npl.ctypes.data_as(C.POINTER(C.c_uint32)), _pf(row)), "agz_pruned_target_of")
    return row, npl[:mv.size]


def visit_target_of(moves, visits, action_space, temperature=1.0):
    """the policy row (action_space + 1 floats, Pass last) of root children (moves[i], visits[i]) under TARGET_VISITS (target.hpp;
    host only): what the device records for a root whose read-back is (moves, visits)"""
    mv = np.ascontiguousarray(moves, dtype=np.int32).reshape(-1)
    vis = np.ascontiguousarray(visits, dtype=np.uint32).reshape(-1)
    assert mv.size == vis.size
    row = np.zeros(max(int(action_space), 0) + 1, np.float32)
    _check(lib().agz_visit_target_of(_pi(mv), vis.ctypes.data_as(C.POINTER(C.c_uint32)), mv.size, int(action_space), temperature, _pf(row)),
           "agz_visit_target_of")
    return row
