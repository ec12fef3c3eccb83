"""ctypes binding of the C ABI in ``include/ltr_hip.h``, ``include/ltr_eval.h``, ``include/ltr_listwise.h``,
``include/ltr_lambdarank.h``, ``include/ltr_longpair.h``, ``include/ltr_lambdarank_long.h``, ``include/ltr_mlp_rows.h``, ``include/ltr_mlp_bf16.h``, ``include/ltr_mlp_wide.h``,
``include/ltr_linear_bf16.h``, ``include/ltr_mlp_train.h`` and ``include/ltr_sched.h`` (pytorchltr_amd/csrc/libltr_hip.so).

PyTorch supplies device memory and the current HIP stream; every call here hands raw device
pointers to the library.  The library must exist -- there is deliberately no fallback.
"""
import ctypes
import os

import torch  # noqa: F401  (loads the HIP runtime the extension binds to, before dlopen)

_HERE = os.path.dirname(os.path.abspath(__file__))
# LTR_HIP_LIB: another build of the same library (tuning variants, scripts/build_variants.sh)
LIB_PATH = os.environ.get("LTR_HIP_LIB") or os.path.join(_HERE, "csrc", "libltr_hip.so")

# enum ltr_loss_kind
HINGE, DCG_HINGE, LOGISTIC, ARP1, ARP2, NDCG1, NDCG2 = range(7)
# enum ltr_label_dtype
LABEL_I64, LABEL_F32, LABEL_I32 = 0, 1, 2
ERR_CONFIG = -6
ERR_TIMEOUT = -7
# ltr_linear_fused_plan (include/ltr_hip.h)
PLAN_NONE, PLAN_REGISTER_TILE, PLAN_CLUSTER, PLAN_GENERAL, PLAN_PARTS = 0, 1, 2, 3, 4

_vp, _i, _f, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t

# name -> (restype, argtypes); mirrors include/ltr_hip.h line by line
SIGNATURES = {
    "ltr_version": (_i, []),
    "ltr_error_string": (ctypes.c_char_p, [_i]),
    "ltr_max_list_len": (_i, []),
    "ltr_max_list_len_f64": (_i, []),
    "ltr_device_status": (_i, [_i]),
    "ltr_debug_force_timeout": (None, [_i]),
    "ltr_debug_cluster_mode": (None, [_i]),
    "ltr_debug_parts_all": (_i, [_i]),
    "ltr_exchange_release": (_i, []),
    "ltr_debug_set_exchange_tag": (_i, [_vp, ctypes.c_uint32]),
    "ltr_debug_stream_probe_f32": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "ltr_debug_kernel_events": (_i, [_vp, _vp]),
    "ltr_debug_mlp_layout": (None, [_i]),
    "ltr_debug_mlp_probe_f32": (_i, [_vp] * 8 + [_i] * 5 + [_vp, _vp]),
    "ltr_pairwise_loss_f32": (_i, [_i, _f, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "ltr_pairwise_loss_f32_cfg": (_i, [_i, _f, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _i, _i, _i, _vp]),
    "ltr_pairwise_loss_workspace_bytes": (_sz, [_i, _i, _i]),
    "ltr_pairwise_loss_ws_f32": (_i, [_i, _f, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "ltr_scale_rows_f32": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "ltr_scale_rows_uniform_f32": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "ltr_pairwise_loss_f64": (_i, [_i, ctypes.c_double, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "ltr_scale_rows_f64": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "ltr_rank_by_score_f32": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "ltr_dcg_f32": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "ltr_arp_f32": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _vp]),
    "ltr_rank_by_score_tie_f32": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "ltr_dcg_tie_f32": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "ltr_arp_tie_f32": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp]),
    "ltr_rank_by_score_seed_f32": (_i, [_vp, _vp, ctypes.c_uint64, _vp, _i, _i, _vp, _vp]),
    "ltr_dcg_seed_f32": (_i, [_vp, _vp, _i, _vp, ctypes.c_uint64, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "ltr_arp_seed_f32": (_i, [_vp, _vp, _i, _vp, ctypes.c_uint64, _vp, _i, _i, _vp, _vp]),
    "ltr_tie_hash_word": (ctypes.c_uint32, [ctypes.c_uint64, ctypes.c_uint32]),
    "ltr_max_sort_list_len": (_i, []),
    "ltr_sort_workspace_bytes": (_sz, [_i, _i, _i]),
    "ltr_rank_by_score_long_f32": (_i, [_vp, _vp, _vp, _i, ctypes.c_uint64, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "ltr_dcg_long_f32": (_i, [_vp, _vp, _i, _vp, _vp, _i, ctypes.c_uint64, _vp, _i, _i, _i, _i, _i, _vp, _vp, _sz,
                              _vp]),
    "ltr_arp_long_f32": (_i, [_vp, _vp, _i, _vp, _vp, _i, ctypes.c_uint64, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "ltr_tie_hash_word_long": (ctypes.c_uint32, [ctypes.c_uint64, ctypes.c_uint32]),
    "ltr_debug_long_sort_all": (_i, [_i]),
    "ltr_listwise_softmax_f32": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "ltr_mask_padded_values_f32": (_i, [_vp, _vp, _i, _i, _f, _vp, _vp]),
    "ltr_batch_pairs": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "ltr_plackettluce_keys_f32": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "ltr_pbm_clicks": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _f, _vp, _vp, _vp]),
    "ltr_collate_pad_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "ltr_collate_pad_csr_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "ltr_linear_workspace_bytes": (_sz, [_i, _i, _i]),
    "ltr_linear_fused_plan": (_i, [_i, _i, _i, _i]),
    "ltr_overlap_create": (_i, [_vp, _vp, _i, _vp]),
    "ltr_overlap_destroy": (_i, [_vp]),
    "ltr_overlap_wait": (_i, [_vp, _i, _vp]),
    "ltr_overlap_flush": (_i, [_vp]),
    "ltr_linear_step_f32": (_i, [_i, _f, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _sz,
                                _vp, _i, _vp]),
    "ltr_linear_sgd_step_f32": (_i, [_i, _f, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _sz,
                                    _vp, _vp]),
    "ltr_linear_sgd_lazy_step_f32": (_i, [_i, _f, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _sz, _i, _vp]),
    "ltr_linear_sgd_flush_f32": (_i, [_i, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp]),
    "ltr_linear_sgd_lazy_step_dp_f32": (_i, [_i, _f, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _sz, _i, _f, _vp, _i, _vp, _vp]),
    "ltr_linear_sgd_flush_dp_f32": (_i, [_i, _vp, _vp, _i, _i, _i, _f, _f, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "ltr_linear_lazy_rows_reduce_f32": (_i, [_i, _i, _i, _i, _f, _vp, _i, _vp, _vp, _vp, _i, _vp]),
    "ltr_debug_fake_allreduce": (_i, [_vp, _vp, _sz, _i, _i, _vp, _vp]),
    "ltr_mailbox_create": (_i, [_i, _i, _i, _vp, _vp]),
    "ltr_mailbox_connect": (_i, [_vp, _vp]),
    "ltr_mailbox_destroy": (_i, [_vp]),
    "ltr_mailbox_allreduce": (_i, [_vp, _vp, _sz, _i, _i, _vp, _vp]),
    "ltr_debug_mailbox_state": (_i, [_vp, ctypes.c_longlong, ctypes.c_longlong]),
    "ltr_mailbox_set_timeout_ms": (ctypes.c_longlong, [ctypes.c_longlong]),
    "ltr_linear_pairwise_f32": (_i, [_i, _f, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i,
                                     _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ltr_linear_partials_f32": (_i, [_i, _f, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i,
                                     _vp, _vp, _vp, _vp]),
    "ltr_linear_reduce_f32": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "ltr_linear_reduce_bcast_f32": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "ltr_linear_reduce_loss_f32": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "ltr_linear_reduce_accum_f32": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp]),
    "ltr_linear_scores_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "ltr_linear_grad_workspace_bytes": (_sz, [_i, _i, _i]),
    "ltr_linear_grad_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ltr_mlp_max_list_len": (_i, [_i]),
    "ltr_mlp_param_count": (_sz, [_i, _i, _i]),
    "ltr_mlp_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "ltr_mlp_scores_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "ltr_mlp_pairwise_f32": (_i, [_i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp,
                                  _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}

# name -> (restype, argtypes); mirrors include/ltr_eval.h (evaluate(): many metrics from one ranking)
EVAL_SIGNATURES = {
    "ltr_eval_workspace_bytes": (_sz, [_i, _i, _vp, _i]),
    "ltr_eval_f32": (_i, [_vp, _vp, _i, _vp, _vp, _i, ctypes.c_uint64, _vp, _i, _i, _vp, _i, _f, _i, _f, _vp, _vp,
                          _sz, _vp]),
}

# enum of include/ltr_listwise.h: the losses of the fused listwise Linear step
LISTWISE_LISTNET, LISTWISE_LISTMLE = 0, 1

# name -> (restype, argtypes); mirrors include/ltr_listwise.h (ListMLE, the fused listwise Linear and MLP steps)
LISTWISE_SIGNATURES = {
    "ltr_listmle_workspace_bytes": (_sz, [_i, _i]),
    "ltr_listmle_f32": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, ctypes.c_uint64, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "ltr_linear_listwise_plan": (_i, [_i, _i, _i, _i]),
    "ltr_linear_listwise_partials_f32": (_i, [_i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, ctypes.c_uint64, _vp, _i, _i, _i,
                                              _vp, _vp, _vp, _vp]),
    "ltr_mlp_listwise_plan": (_i, [_i, _i, _i, _i, _i, _i]),
    "ltr_mlp_listwise_f32": (_i, [_i, _i] + [_vp] * 7 + [_vp, _i, _vp, _vp, _i, ctypes.c_uint64, _vp, _vp]
                             + [_i] * 5 + [_vp] * 5 + [_sz, _vp]),
}

# LambdaRank as a loss of the fused listwise Linear step: a Python-side code next to the two above (the library's
# entry points for it are their own, below; ltr_linear_listwise_* answer LTR_ERR_KIND / 0 for it)
LISTWISE_LAMBDARANK = 2

# name -> (restype, argtypes); mirrors include/ltr_lambdarank.h (LambdaRank with NDCG@k swap weights, its fused Linear step)
LAMBDARANK_SIGNATURES = {
    "ltr_lambdarank_f32": (_i, [_vp, _vp, _i, _vp, _i, _f, _i, _i, _vp, _vp, _vp]),
    "ltr_linear_lambdarank_plan": (_i, [_i, _i, _i]),
    "ltr_linear_lambdarank_partials_f32": (_i, [_i, _f, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); mirrors include/ltr_mlp_lambdarank.h (the fused MLP step with LambdaRank in its loss slot)
MLP_LAMBDARANK_SIGNATURES = {
    "ltr_mlp_lambdarank_plan": (_i, [_i, _i, _i, _i, _i]),
    "ltr_mlp_lambdarank_f32": (_i, [_i, _f] + [_vp] * 7 + [_vp, _i, _vp, _vp] + [_i] * 5 + [_vp] * 5 + [_sz, _vp]),
}

# include/ltr_mlp_train.h: the update rules, the loss families of a step and the hyper-parameter struct
OPT_SGD, OPT_ADAGRAD, OPT_ADAM = 0, 1, 2
MLP_TRAIN_PAIRWISE, MLP_TRAIN_LISTWISE, MLP_TRAIN_LAMBDARANK = 0, 1, 2


class MLPOptim(ctypes.Structure):
    """``struct ltr_mlp_optim``."""
    _fields_ = [("algo", _i), ("nesterov", _i)] + [(name, ctypes.c_double) for name in (
        "lr", "weight_decay", "momentum", "dampening", "lr_decay", "eps", "beta1", "beta2")]


_optp = ctypes.POINTER(MLPOptim)

# name -> (restype, argtypes); mirrors include/ltr_mlp_train.h (the fused MLP step with the optimizer update in-launch)
MLP_TRAIN_SIGNATURES = {
    "ltr_mlp_train_state_floats": (_sz, [_i, _i, _i, _i]),
    "ltr_mlp_train_step_f32": (_i, [_i, _i, _i, _f] + [_vp] * 7 + [_i, _vp, _vp, _i, _vp, _vp, _i, ctypes.c_uint64, _vp, _vp]
                               + [_i] * 5 + [_vp] * 4 + [_optp, _vp, _vp, _sz, _vp]),
    "ltr_mlp_apply_update_f32": (_i, [_vp] * 7 + [_i, _vp, _optp, _i, _i, _i, _vp]),
}

# name -> (restype, argtypes); mirrors include/ltr_mlp_rows.h (the MLP scorer on its own: scores and gradients, any length)
MLP_ROWS_SIGNATURES = {
    "ltr_mlp_rows_scores_f32": (_i, [_vp] * 8 + [_i] * 5 + [_vp, _vp]),
    "ltr_mlp_rows_grad_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "ltr_mlp_rows_grad_f32": (_i, [_vp] * 9 + [_i] * 5 + [_vp, _vp, _sz, _vp]),
}

# name -> (restype, argtypes); mirrors include/ltr_mlp_bf16.h (the same scorer on a bf16 feature batch, bf16 MFMA layer 1)
MLP_BF16_SIGNATURES = {
    "ltr_mlp_bf16_scores": (_i, [_vp] * 8 + [_i] * 5 + [_vp, _vp]),
    "ltr_mlp_bf16_grad_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "ltr_mlp_bf16_grad": (_i, [_vp] * 9 + [_i] * 5 + [_vp, _vp, _sz, _vp]),
}

# name -> (restype, argtypes); mirrors include/ltr_linear_bf16.h (the Linear(F, 1) scorer on a bf16 feature batch: the
# streaming score / gradient kernels, the fused register-tile step and its plan, the bf16 collate)
LINEAR_BF16_SIGNATURES = {
    "ltr_linear_scores_bf16": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "ltr_linear_grad_workspace_bytes_bf16": (_sz, [_i, _i, _i]),
    "ltr_linear_grad_bf16": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ltr_linear_bf16_plan": (_i, [_i, _i, _i, _i]),
    "ltr_linear_partials_bf16": (_i, [_i, _f, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "ltr_collate_pad_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); mirrors include/ltr_mlp_wide.h (the same scorer on rows of up to 704 features)
MLP_WIDE_SIGNATURES = {
    "ltr_mlp_wide_scores_f32": (_i, [_vp] * 8 + [_i] * 5 + [_vp, _vp]),
    "ltr_mlp_wide_grad_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "ltr_mlp_wide_grad_f32": (_i, [_vp] * 9 + [_i] * 5 + [_vp, _vp, _sz, _vp]),
}

# name -> (restype, argtypes); mirrors include/ltr_longpair.h (the pairwise losses past max_list_len() documents)
LONGPAIR_SIGNATURES = {
    "ltr_max_pair_list_len": (_i, []),
    "ltr_long_pair_geometry": (None, [_vp, _vp]),
    "ltr_pairwise_loss_long_workspace_bytes": (_sz, [_i, _i, _i]),
    "ltr_pairwise_loss_long_f32": (_i, [_i, _f, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "ltr_debug_long_pairs_all": (_i, [_i]),
}

# name -> (restype, argtypes); mirrors include/ltr_lambdarank_long.h (LambdaRank past max_list_len() documents)
LAMBDARANK_LONG_SIGNATURES = {
    "ltr_lambdarank_long_workspace_bytes": (_sz, [_i, _i, _i]),
    "ltr_lambdarank_long_f32": (_i, [_vp, _vp, _i, _vp, _i, _f, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "ltr_debug_lambdarank_long_all": (_i, [_i]),
}

# name -> (restype, argtypes); mirrors include/ltr_sched.h (hooks of the list-length scheduling and the lazy launch's hold-backs)
SCHED_SIGNATURES = {
    "ltr_debug_sched_slots": (_i, [_i, _i, _i, _i, _vp, _vp]),
    "ltr_debug_sched_slots_cu": (_i, [_i, _i, _i, _i, _i, _vp, _vp]),
    "ltr_debug_lazy_holdback": (_i, [_i]),
}

_lib = None


class ExtensionMissingError(ImportError):
    pass


class _Library(ctypes.CDLL):
    """ctypes.CDLL that says WHY a test / tuning hook is missing: a production build (LTR_NO_DEBUG_HOOKS=1) does not
    export the ltr_debug_* entry points (the bare AttributeError came up far from its cause)."""

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if name.startswith("ltr_debug_"):
                raise AttributeError(
                    "%s is a test / tuning hook and this libltr_hip.so was built without them (LTR_NO_DEBUG_HOOKS=1); "
                    "rebuild with `python -m pytorchltr_amd.build --force` and the variable unset" % name) from None
            raise


def lib():
    """The loaded extension.  Raises loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ExtensionMissingError(
                "pytorchltr_amd HIP extension not found at %s; build it with "
                "`python -m pytorchltr_amd.build` (hipcc --offload-arch=gfx950). "
                "There is no CPU fallback." % LIB_PATH)
        handle = _Library(LIB_PATH)
        for name, (restype, argtypes) in (list(SIGNATURES.items()) + list(EVAL_SIGNATURES.items())
                                          + list(LISTWISE_SIGNATURES.items()) + list(LAMBDARANK_SIGNATURES.items())
                                          + list(LONGPAIR_SIGNATURES.items()) + list(LAMBDARANK_LONG_SIGNATURES.items())
                                          + list(MLP_LAMBDARANK_SIGNATURES.items()) + list(MLP_TRAIN_SIGNATURES.items())
                                          + list(MLP_ROWS_SIGNATURES.items()) + list(MLP_WIDE_SIGNATURES.items())
                                          + list(MLP_BF16_SIGNATURES.items()) + list(LINEAR_BF16_SIGNATURES.items())
                                          + list(SCHED_SIGNATURES.items())):
            if name.startswith("ltr_debug_") and not hasattr(handle, name):
                continue                     # a production build (-DLTR_NO_DEBUG_HOOKS) leaves the test hooks out
            fn = getattr(handle, name)       # AttributeError if the symbol is missing
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
    return _lib


def check(rc):
    if rc != 0:
        msg = lib().ltr_error_string(int(rc))
        raise RuntimeError("pytorchltr_amd: %s (code %d)" % (msg.decode() if msg else "?", rc))


def ptr(t):
    return None if t is None else t.data_ptr()


try:                                    # raw stream handle without building a Stream object
    _raw_stream = torch._C._cuda_getCurrentRawStream
except AttributeError:                  # pragma: no cover - older/newer torch
    _raw_stream = None


def stream_of(t):
    """hipStream_t (as int) of torch's current stream on t's device."""
    if _raw_stream is not None:
        return _raw_stream(t.device.index if t.device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(t.device).cuda_stream


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NULL = _NullCtx()


def device_ctx(t):
    """Context that makes t's device current for the launch; free when it already is."""
    idx = t.device.index
    if idx is None or idx == torch.cuda.current_device():
        return _NULL
    return torch.cuda.device(idx)


_max_len = None
_max_len_f64 = None


def max_list_len():
    global _max_len
    if _max_len is None:
        _max_len = int(lib().ltr_max_list_len())
    return _max_len


_max_pair_len = None


def max_pair_list_len():
    """Longest list the pairwise losses take with ``long_lists=True`` (ltr_max_pair_list_len)."""
    global _max_pair_len
    if _max_pair_len is None:
        _max_pair_len = int(lib().ltr_max_pair_list_len())
    return _max_pair_len


def long_pair_geometry():
    """(owner_docs, chunk_docs) of the long pairwise path: documents per workgroup, documents per LDS chunk."""
    own, ch = ctypes.c_int(0), ctypes.c_int(0)
    lib().ltr_long_pair_geometry(ctypes.byref(own), ctypes.byref(ch))
    return own.value, ch.value


_max_sort_len = None


def max_sort_list_len():
    """Longest list the rankings and metrics take (their long path; the losses stop at max_list_len())."""
    global _max_sort_len
    if _max_sort_len is None:
        _max_sort_len = int(lib().ltr_max_sort_list_len())
    return _max_sort_len


def workspace(nbytes, device):
    """A workspace of `nbytes` bytes on `device` for an ltr_*_workspace_bytes count: (tensor, bytes), or (None, 0)
    where the entry point needs none."""
    nbytes = int(nbytes)
    return (torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes > 0 else None), nbytes


def sort_workspace(op, B, L, device):
    """Workspace of the ltr_*_long_f32 entry points (op 0 rank, 1 dcg / ndcg, 2 arp): (tensor, bytes).
    (None, 0) for lists of at most max_list_len(): the entry points do not read it there."""
    return workspace(lib().ltr_sort_workspace_bytes(op, B, L) if L > max_list_len() else 0, device)


def max_list_len_f64():
    global _max_len_f64
    if _max_len_f64 is None:
        _max_len_f64 = int(lib().ltr_max_list_len_f64())
    return _max_len_f64


def device_status(clear=True, synchronize=True):
    """The sticky device status word (include/ltr_hip.h: ltr_device_status): raises RuntimeError if
    a multi-workgroup kernel of an earlier launch gave up waiting for its partners (its outputs are
    NaN-poisoned).  `synchronize` waits for the current device first, so the answer covers every
    launch issued so far."""
    if synchronize and torch.cuda.is_available():
        torch.cuda.synchronize()
    check(lib().ltr_device_status(1 if clear else 0))


def require_device(t, what):
    if not t.is_cuda:
        raise RuntimeError(
            "pytorchltr_amd: `%s` is on %s; this library only runs its HIP kernels on a ROCm "
            "device (no CPU fallback). Move the batch with .to('cuda')." % (what, t.device))


def label_dtype(rel):
    if rel.dtype == torch.int64:
        return LABEL_I64
    if rel.dtype == torch.float32:
        return LABEL_F32
    if rel.dtype == torch.int32:
        return LABEL_I32
    raise TypeError("unsupported relevance dtype %s" % rel.dtype)
