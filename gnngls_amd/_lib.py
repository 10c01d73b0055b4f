"""ctypes binding of libgnngls_hip.so (C ABI declared in include/gnngls_hip.h).

The product path has no CPU fallback: if the HIP library is missing or a call fails, this raises.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# GNNGLS_HIP_SO: another build of the same library (A/B kernel experiments, diagnostic -DGLS_STAMPS builds)
SO = os.environ.get("GNNGLS_HIP_SO") or os.path.join(HERE, "libgnngls_hip.so")

_vp = ctypes.c_void_p
_int = ctypes.c_int
_i64 = ctypes.c_int64
_f64 = ctypes.c_double
_f32 = ctypes.c_float
_u64 = ctypes.c_uint64

# name -> argtypes; every function returns int (0 = ok) unless listed in _RESTYPES
SIGNATURES = {
    "gnngls_abi_version": [],
    "gnngls_last_error": [],
    "gnngls_gls_resident_capacity": [_int],
    "gnngls_gls_describe_config": [_int, _int, _int, _vp, _vp, _vp, _vp],
    "gnngls_gls_describe_run": [_int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "gnngls_gls_kernel_resources": [_int, _int, _int, _int, _int, _vp, _vp],
    "gnngls_two_opt_delta_all": [_vp, _vp, _int, _int, _vp, _vp],
    "gnngls_relocate_delta_all": [_vp, _vp, _int, _int, _vp, _vp],
    "gnngls_best_move": [_vp, _vp, _int, _int, _int, _vp, _int, _vp, _vp, _vp, _vp],
    "gnngls_tour_cost": [_vp, _vp, _int, _int, _vp, _vp],
    "gnngls_nearest_neighbor": [_vp, _int, _int, _int, _vp, _vp],
    "gnngls_insertion": [_vp, _int, _int, _int, _int, _vp, _vp, _vp, _vp],
    "gnngls_cheapest_insertion": [_vp, _int, _vp, _vp, _int, _int, _vp, _vp, _vp],
    "gnngls_one_tree_bound": [_vp, _vp, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp],
    "gnngls_one_tree_bound_describe": [_int, _vp, _vp, _vp],
    "gnngls_alpha_nearness": [_vp, _vp, _int, _int, _vp, _vp, _vp],
    "gnngls_or_opt_best_move": [_vp, _vp, _int, _int, _int, _int, _vp, _vp, _vp, _vp],
    "gnngls_or_opt_descent": [_vp, _vp, _vp, _int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _int, _vp],
    "gnngls_ils_run": [_vp, _vp, _vp, _int, _int, _int, _int, _int, _int, _int, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "gnngls_or_opt_o2a": [_vp, _vp, _vp, _int, _int, _int, _int, _vp, _vp, _vp, _vp],
    "gnngls_guided_or_opt_run": [_vp, _vp, _vp, _vp, _int, _vp, _vp, _int, _int, _int, _int, _int, _int, _int, _int, _int,
                                 _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp],
    "gnngls_three_opt_best_move": [_vp, _vp, _int, _int, _vp, _vp, _vp, _vp],
    "gnngls_three_opt_descent": [_vp, _vp, _vp, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _int, _vp],
    "gnngls_three_opt_lds_max_n": [],
    "gnngls_sample_nn_tours": [_vp, _int, _int, _int, _int, _int, _u64, _vp, _vp, _vp, _vp],
    "gnngls_aco_run": [_vp, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _i64, _f64, _f64, _int, _int, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "gnngls_beam_search_workspace_bytes": [_int, _int, _int],
    "gnngls_beam_search": [_vp, _vp, _int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    "gnngls_greedy_edge": [_vp, _vp, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "gnngls_gls_run": [_vp, _vp, _int, _int, _int, _vp, _vp, _int, _int, _int, _i64, _f64, _f64,
                       _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp],
    "gnngls_model_packed_floats": [_int, _int],
    "gnngls_regret_forward_workspace_bytes": [_int, _int],
    "gnngls_regret_forward": [_vp, _vp, _int, _int, _int, _int, _vp, _vp, _i64, _vp],
    "gnngls_regret_prepared_bytes": [_int],
    "gnngls_regret_prepare": [_vp, _int, _int, _vp, _i64, _vp],
    "gnngls_regret_forward_prepared": [_vp, _vp, _vp, _i64, _int, _int, _int, _int, _vp, _vp, _i64, _vp],
    "gnngls_regret_train_workspace_bytes": [_int, _int, _int],
    "gnngls_regret_train_forward": [_vp, _vp, _int, _int, _int, _int, _f32, _vp, _vp, _vp, _i64, _vp],
    "gnngls_regret_train_backward": [_vp, _vp, _vp, _int, _int, _int, _int, _vp, _vp, _i64, _vp],
    "gnngls_model_heads_supported": [_int],
    "gnngls_regret_forward_workspace_bytes_heads": [_int, _int, _int],
    "gnngls_regret_forward_heads": [_vp, _vp, _int, _int, _int, _int, _int, _vp, _vp, _i64, _vp],
    "gnngls_regret_prepare_heads": [_vp, _int, _int, _int, _vp, _i64, _vp],
    "gnngls_regret_forward_prepared_heads": [_vp, _vp, _vp, _i64, _int, _int, _int, _int, _int, _vp, _vp, _i64, _vp],
    "gnngls_regret_train_workspace_bytes_heads": [_int, _int, _int, _int],
    "gnngls_regret_train_forward_heads": [_vp, _vp, _int, _int, _int, _int, _int, _f32, _vp, _vp, _vp, _i64, _vp],
    "gnngls_regret_train_backward_heads": [_vp, _vp, _vp, _int, _int, _int, _int, _int, _vp, _vp, _i64, _vp],
    "gnngls_pack_features": [_vp, _int, _int, _f64, _f64, _vp, _vp],
    "gnngls_unpack_regret": [_vp, _int, _int, _f64, _f64, _vp, _vp],
    "gnngls_debug_set_penalty16_limit": [_int],
    "gnngls_debug_set_stamp_buffer": [_vp],
    "gnngls_debug_set_gls_threads": [_int],
    "gnngls_debug_set_gls_team": [_int],
    "gnngls_debug_set_gls_prune": [_int],
    "gnngls_gls_uses_team": [_int, _int, _int],
    "gnngls_gls_waves_per_simd": [_int, _int, _int],
    "gnngls_profile_enable": [_int],
    "gnngls_profile_collect": [_vp, _vp],
    "gnngls_profile_set_executed_evals": [_vp],
    "gnngls_regret_labels_chunk": [_int],
    "gnngls_regret_labels": [_vp, _int, _int, _vp, _vp, _int, _i64, _int, _f64, _int, _vp, _vp, _vp, _vp, _vp, _vp],
}

PROF_KINDS = ["pack_features", "embed", "gemm_fc", "gat_rows", "gat_rows_rank1", "gemm_ffn1(unused)", "gemm_ffn2(unused)",
              "decision", "unpack_regret", "nearest_neighbor", "tour_cost", "gls", "ffn_fused",
              "train_colsum", "train_elementwise", "train_gemm_bwd", "train_gemm_tn", "train_gat_bwd", "insertion"]
# kinds of entries added after the constructors (GNNGLS_PROF_* in the header's order, behind PROF_KINDS: no index moved)
PROF_KINDS_BOUNDS = ["one_tree_bound"]


def profile_enable(on=True):
    check(load().gnngls_profile_enable(int(on)), "profile_enable")


def profile_collect():
    """-> {kind: (milliseconds, launches)} since profile_enable(True)."""
    kinds = PROF_KINDS + (PROF_KINDS_BOUNDS if hasattr(load(), "gnngls_one_tree_bound") else [])
    n = len(kinds)
    ms = (ctypes.c_double * n)()
    cnt = (ctypes.c_int64 * n)()
    check(load().gnngls_profile_collect(ctypes.cast(ms, ctypes.c_void_p), ctypes.cast(cnt, ctypes.c_void_p)),
          "profile_collect")
    return {k: (ms[i], cnt[i]) for i, k in enumerate(kinds)}
_RESTYPES = {"gnngls_last_error": ctypes.c_char_p, "gnngls_model_packed_floats": ctypes.c_int64,
             "gnngls_regret_forward_workspace_bytes": ctypes.c_int64,
             "gnngls_regret_prepared_bytes": ctypes.c_int64,
             "gnngls_regret_train_workspace_bytes": ctypes.c_int64,
             "gnngls_regret_forward_workspace_bytes_heads": ctypes.c_int64,
             "gnngls_regret_train_workspace_bytes_heads": ctypes.c_int64,
             "gnngls_beam_search_workspace_bytes": ctypes.c_int64}

_ABI4 = ("gnngls_regret_prepared_bytes", "gnngls_regret_prepare", "gnngls_regret_forward_prepared")
# head counts other than 8 (an older build named by GNNGLS_HIP_SO lacks them; the 8-head path never calls them)
_HEADS = ("gnngls_model_heads_supported", "gnngls_regret_forward_workspace_bytes_heads", "gnngls_regret_forward_heads",
          "gnngls_regret_prepare_heads", "gnngls_regret_forward_prepared_heads", "gnngls_regret_train_workspace_bytes_heads",
          "gnngls_regret_train_forward_heads", "gnngls_regret_train_backward_heads")
# the insertion tour constructors (an older build named by GNNGLS_HIP_SO lacks them; ops.insertion then raises)
_CONSTRUCTORS = ("gnngls_insertion", "gnngls_cheapest_insertion")
# the Held-Karp 1-tree bound (an older build named by GNNGLS_HIP_SO lacks it; ops.one_tree_bound then raises)
_BOUNDS = ("gnngls_one_tree_bound", "gnngls_one_tree_bound_describe")
# the sampled nearest-neighbour walks (an older build named by GNNGLS_HIP_SO lacks them; ops.sample_nn_tours then raises)
_SAMPLING = ("gnngls_sample_nn_tours",)
# alpha-nearness (an older build named by GNNGLS_HIP_SO lacks it; ops.alpha_nearness then raises)
_ALPHA = ("gnngls_alpha_nearness",)
# Or-opt (an older build named by GNNGLS_HIP_SO lacks it; ops.or_opt_best_move / or_opt_descent then raise)
_OR_OPT = ("gnngls_or_opt_best_move", "gnngls_or_opt_descent")
# iterated local search (an older build named by GNNGLS_HIP_SO lacks it; ops.ils then raises)
_ILS = ("gnngls_ils_run",)
# 3-opt (an older build named by GNNGLS_HIP_SO lacks it; ops.three_opt_best_move / three_opt_descent then raise)
_THREE_OPT = ("gnngls_three_opt_best_move", "gnngls_three_opt_descent", "gnngls_three_opt_lds_max_n")
# guided local search over 2-opt and Or-opt (an older build named by GNNGLS_HIP_SO lacks it; ops.or_opt_o2a / guided_or_opt then raise)
_GUIDED_OR_OPT = ("gnngls_or_opt_o2a", "gnngls_guided_or_opt_run")
# the ant system (an older build named by GNNGLS_HIP_SO lacks it; ops.aco then raises)
_ACO = ("gnngls_aco_run",)
# beam search (an older build named by GNNGLS_HIP_SO lacks it; ops.beam_search then raises)
_BEAM = ("gnngls_beam_search", "gnngls_beam_search_workspace_bytes")
# greedy edge matching (an older build named by GNNGLS_HIP_SO lacks it; ops.greedy_edge then raises)
_GREEDY_EDGE = ("gnngls_greedy_edge",)
_lib = None


class GnnglsHipError(RuntimeError):
    pass


def load():
    """Loads the shared library (building nothing: run `python -m gnngls_amd.build` or
    __graft_entry__.build() first).  Raises if it is absent -- there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.isfile(SO):
            raise GnnglsHipError(
                f"{SO} not found: build the HIP extension with `python -m gnngls_amd.build` "
                "(this package has no CPU fallback)")
        # PyTorch-ROCm bundles its own libamdhip64.so.7 (same SONAME as /opt/rocm's).  The process must
        # hold exactly ONE HIP runtime, and it has to be the one torch's streams/allocations live in:
        # import torch first so the dynamic linker binds this library to the runtime torch loaded.
        import torch  # noqa: F401
        L = ctypes.CDLL(SO)
        for name, argtypes in SIGNATURES.items():
            if (name in _ABI4 or name in _HEADS or name in _CONSTRUCTORS or name in _BOUNDS or name in _SAMPLING or name in _ALPHA or name in _OR_OPT or name in _ILS or name in _THREE_OPT or name in _GUIDED_OR_OPT or name in _ACO or name in _BEAM or name in _GREEDY_EDGE) and "GNNGLS_HIP_SO" in os.environ and not hasattr(L, name):
                continue              # an older build of the library named by GNNGLS_HIP_SO (same-box A/B of kernel variants)
            f = getattr(L, name)      # AttributeError if the symbol is missing
            f.argtypes = argtypes
            f.restype = _RESTYPES.get(name, ctypes.c_int)
        _lib = L
    return _lib


def check(code, what=""):
    if code != 0:
        msg = load().gnngls_last_error()
        raise GnnglsHipError(f"{what} failed ({code}): {msg.decode() if msg else ''}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensor required"
    return ctypes.c_void_p(t.data_ptr())


def current_stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
