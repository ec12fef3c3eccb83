"""The route table of the Linear(F, 1) scorer: which entry points a batch reaches from each public caller.

CASES varies one axis at a time off two bases (fp32, F = 8, L = 5, n = [L, L // 2 + 1, ...], contiguous, bias, no input
gradient, no autocast; B = 2 and B = 160, on each side of the few-lists rule 2 B <= CUs), plus the crossings on each side of
every limit of the table.  EXPECTED is what tests/test_gpu_linear_routes.py recorded on an MI355X at commit e49dee3 (the
parent of the commit that folded the routes into ``fused._linear_route``): per case and caller, the entry points in the
order they were called, "torch" where ``LinearScorer`` fell back to ``torch.nn.functional.linear``, "raises <class>" where
the call raised.  ANSWERS is what the library answered there where the route function takes its answer as a plain value
(the CU count, ``ltr_linear_fused_plan`` at F and at F rounded up to 4, ``ltr_linear_listwise_plan`` on the rows as they
lie in memory); the GPU test asserts that they still are the library's.  The GPU test proves that the callers obey the
table; the tests below prove, without a GPU, that the one pure route function states it.
"""
import pytest
import torch

MAX_LIST_LEN = 4096                 # ltr_max_list_len(): asserted by the test below and by the GPU tier
BASE = dict(dtype="float32", B=2, L=5, F=8, view=None, xgrad=False, autocast=False, cpu=False, bias=True,
            wrong_weight=False)


def _vary(**kw):
    return dict(BASE, **kw)


CASES = {
    "base": _vary(), "base160": _vary(B=160),
    "bf16": _vary(dtype="bfloat16"), "bf16-160": _vary(dtype="bfloat16", B=160),
    "fp16": _vary(dtype="float16"), "fp64": _vary(dtype="float64"),
    "F5": _vary(F=5), "F46": _vary(F=46), "F136": _vary(F=136), "bf16-F12": _vary(dtype="bfloat16", F=12),
    # views and strides
    "ragged4": _vary(F=5, view="ragged"), "bf16-ragged8": _vary(dtype="bfloat16", F=12, view="ragged"),
    "strided": _vary(F=5, view="strided"), "offset": _vary(view="offset"), "bf16-offset": _vary(dtype="bfloat16", view="offset"),
    # batch flags and parameters
    "xgrad": _vary(xgrad=True), "autocast": _vary(autocast=True), "cpu": _vary(cpu=True), "nobias": _vary(bias=False),
    "B0": _vary(B=0), "wrong-weight": _vary(wrong_weight=True),
    # the few-lists rule where the stand-alone loss has a split-query form (fp32, L = 400: its workspace is not empty);
    # at the longest list of the bf16 tile it has none, and the bf16 step stays fused
    "few-lists": _vary(L=400), "bf16-few-lists": _vary(dtype="bfloat16", L=256),
    # L around the bf16 tile limit
    "bf16-F136-L256": _vary(dtype="bfloat16", B=160, F=136, L=256), "bf16-F136-L257": _vary(dtype="bfloat16", B=160, F=136, L=257),
    "bf16-F704-L80": _vary(dtype="bfloat16", B=160, F=704, L=80), "bf16-F704-L81": _vary(dtype="bfloat16", B=160, F=704, L=81),
    # the heavy-pairs rule (B <= CUs and L > 768, not for the hinge kinds)
    "B160-L768": _vary(B=160, L=768), "B160-L769": _vary(B=160, L=769),
    # the cluster / parts exemption: 32 x 1000 x 220 and 64 x 512 x 700 shrunk as far as the plan answers the same
    "cluster": _vary(L=400, F=64), "parts": _vary(L=600), "B80-L500-F512": _vary(B=80, L=500, F=512),
    # past max_list_len() (the callers "...-long" pass long_lists=True)
    "long": _vary(L=MAX_LIST_LEN + 4), "bf16-long": _vary(dtype="bfloat16", L=MAX_LIST_LEN + 4),
}

LOSSES = ("hinge", "logistic", "ndcg2", "listnet", "listmle")

# caller -> (what it is, loss): "module" FusedLinearLoss; "lazy" / "eager" a loss module on LinearScorer(F)(xs, n) /
# LinearScorer(F, lazy=False)(xs, n); "step" linear_loss_step; "...-long" the same with a loss module built with
# long_lists=True; "nograd" LinearScorer under no_grad; "lazysgd" two LazySGD steps and flush(); "loop" two steps of the
# user's loop with optim.SGD on a use_linear_scorer model, and its flush
CALLERS = {
    "module-hinge": ("module", "hinge"), "module-logistic": ("module", "logistic"), "module-ndcg2": ("module", "ndcg2"),
    "module-listnet": ("module", "listnet"), "module-listmle": ("module", "listmle"), "module-hinge+scores": ("module", "hinge"),
    "lazy-hinge": ("lazy", "hinge"), "lazy-logistic": ("lazy", "logistic"), "lazy-listnet": ("lazy", "listnet"),
    "eager-hinge": ("eager", "hinge"), "eager-listnet": ("eager", "listnet"),
    "nograd": ("nograd", None),
    "step-hinge": ("step", "hinge"), "step-ndcg2": ("step", "ndcg2"), "step-listnet": ("step", "listnet"),
    "step-listmle": ("step", "listmle"),
    "module-long": ("module-long", "hinge"), "lazy-long": ("lazy-long", "hinge"), "step-long": ("step-long", "hinge"),
    "lazysgd": ("lazysgd", "hinge"), "loop": ("loop", "hinge"),
}


def f4(F):
    return (F + 3) & ~3


def rows_in_memory(case):
    """The row width of the case's batch once it is fp32 on the device: a marked fp32 view keeps its padded rows."""
    return f4(case["F"]) if case["view"] == "ragged" and case["dtype"] == "float32" else case["F"]


# what the library answered on the MI355X at e49dee3 (see the module docstring)
ANSWERS = {
    "base": {"cus": 256, "fused_plan": {"hinge": [1, 1], "logistic": [1, 1], "ndcg2": [1, 1]},
            "listwise_plan": {"listnet": 1, "listmle": 1}},
    "base160": {"cus": 256, "fused_plan": {"hinge": [1, 1], "logistic": [1, 1], "ndcg2": [1, 1]},
               "listwise_plan": {"listnet": 1, "listmle": 1}},
    "bf16": {"cus": 256, "fused_plan": {"hinge": [1, 1], "logistic": [1, 1], "ndcg2": [1, 1]},
            "listwise_plan": {"listnet": 1, "listmle": 1}},
    "bf16-160": {"cus": 256, "fused_plan": {"hinge": [1, 1], "logistic": [1, 1], "ndcg2": [1, 1]},
                "listwise_plan": {"listnet": 1, "listmle": 1}},
    "fp16": {"cus": 256, "fused_plan": {"hinge": [1, 1], "logistic": [1, 1], "ndcg2": [1, 1]},
            "listwise_plan": {"listnet": 1, "listmle": 1}},
    "fp64": {"cus": 256, "fused_plan": {"hinge": [1, 1], "logistic": [1, 1], "ndcg2": [1, 1]},
            "listwise_plan": {"listnet": 1, "listmle": 1}},
    "F5": {"cus": 256, "fused_plan": {"hinge": [3, 1], "logistic": [3, 1], "ndcg2": [3, 1]},
          "listwise_plan": {"listnet": 0, "listmle": 0}},
    "F46": {"cus": 256, "fused_plan": {"hinge": [3, 1], "logistic": [3, 1], "ndcg2": [3, 1]},
           "listwise_plan": {"listnet": 0, "listmle": 0}},
    "F136": {"cus": 256, "fused_plan": {"hinge": [1, 1], "logistic": [1, 1], "ndcg2": [1, 1]},
            "listwise_plan": {"listnet": 1, "listmle": 1}},
    "bf16-F12": {"cus": 256, "fused_plan": {"hinge": [1, 1], "logistic": [1, 1], "ndcg2": [1, 1]},
                "listwise_plan": {"listnet": 1, "listmle": 1}},
    "ragged4": {"cus": 256, "fused_plan": {"hinge": [3, 1], "logistic": [3, 1], "ndcg2": [3, 1]},
               "listwise_plan": {"listnet": 1, "listmle": 1}},
    "bf16-ragged8": {"cus": 256, "fused_plan": {"hinge": [1, 1], "logistic": [1, 1], "ndcg2": [1, 1]},
                    "listwise_plan": {"listnet": 1, "listmle": 1}},
    "strided": {"cus": 256, "fused_plan": {"hinge": [3, 1], "logistic": [3, 1], "ndcg2": [3, 1]},
               "listwise_plan": {"listnet": 0, "listmle": 0}},
    "offset": {"cus": 256, "fused_plan": {"hinge": [1, 1], "logistic": [1, 1], "ndcg2": [1, 1]},
              "listwise_plan": {"listnet": 1, "listmle": 1}},
    "bf16-offset": {"cus": 256, "fused_plan": {"hinge": [1, 1], "logistic": [1, 1], "ndcg2": [1, 1]},
                   "listwise_plan": {"listnet": 1, "listmle": 1}},
    "xgrad": {"cus": 256, "fused_plan": {"hinge": [1, 1], "logistic": [1, 1], "ndcg2": [1, 1]},
             "listwise_plan": {"listnet": 1, "listmle": 1}},
    "autocast": {"cus": 256, "fused_plan": {"hinge": [1, 1], "logistic": [1, 1], "ndcg2": [1, 1]},
                "listwise_plan": {"listnet": 1, "listmle": 1}},
    "cpu": {"cus": 256, "fused_plan": {"hinge": [1, 1], "logistic": [1, 1], "ndcg2": [1, 1]},
           "listwise_plan": {"listnet": 1, "listmle": 1}},
    "nobias": {"cus": 256, "fused_plan": {"hinge": [1, 1], "logistic": [1, 1], "ndcg2": [1, 1]},
              "listwise_plan": {"listnet": 1, "listmle": 1}},
    "B0": {"cus": 256, "fused_plan": {"hinge": [0, 0], "logistic": [0, 0], "ndcg2": [0, 0]},
          "listwise_plan": {"listnet": 0, "listmle": 0}},
    "wrong-weight": {"cus": 256, "fused_plan": {"hinge": [1, 1], "logistic": [1, 1], "ndcg2": [1, 1]},
                    "listwise_plan": {"listnet": 1, "listmle": 1}},
    "few-lists": {"cus": 256, "fused_plan": {"hinge": [3, 3], "logistic": [3, 3], "ndcg2": [3, 3]},
                 "listwise_plan": {"listnet": 1, "listmle": 1}},
    "bf16-few-lists": {"cus": 256, "fused_plan": {"hinge": [1, 1], "logistic": [1, 1], "ndcg2": [1, 1]},
                      "listwise_plan": {"listnet": 1, "listmle": 1}},
    "bf16-F136-L256": {"cus": 256, "fused_plan": {"hinge": [1, 1], "logistic": [1, 1], "ndcg2": [1, 1]},
                      "listwise_plan": {"listnet": 1, "listmle": 1}},
    "bf16-F136-L257": {"cus": 256, "fused_plan": {"hinge": [2, 2], "logistic": [2, 2], "ndcg2": [2, 2]},
                      "listwise_plan": {"listnet": 1, "listmle": 1}},
    "bf16-F704-L80": {"cus": 256, "fused_plan": {"hinge": [3, 3], "logistic": [3, 3], "ndcg2": [3, 3]},
                     "listwise_plan": {"listnet": 1, "listmle": 1}},
    "bf16-F704-L81": {"cus": 256, "fused_plan": {"hinge": [3, 3], "logistic": [3, 3], "ndcg2": [3, 3]},
                     "listwise_plan": {"listnet": 1, "listmle": 1}},
    "B160-L768": {"cus": 256, "fused_plan": {"hinge": [3, 3], "logistic": [3, 3], "ndcg2": [4, 4]},
                 "listwise_plan": {"listnet": 1, "listmle": 1}},
    "B160-L769": {"cus": 256, "fused_plan": {"hinge": [3, 3], "logistic": [3, 3], "ndcg2": [4, 4]},
                 "listwise_plan": {"listnet": 1, "listmle": 1}},
    "cluster": {"cus": 256, "fused_plan": {"hinge": [2, 2], "logistic": [2, 2], "ndcg2": [2, 2]},
               "listwise_plan": {"listnet": 1, "listmle": 1}},
    "parts": {"cus": 256, "fused_plan": {"hinge": [3, 3], "logistic": [3, 3], "ndcg2": [4, 4]},
             "listwise_plan": {"listnet": 1, "listmle": 1}},
    "B80-L500-F512": {"cus": 256, "fused_plan": {"hinge": [2, 2], "logistic": [2, 2], "ndcg2": [3, 3]},
                     "listwise_plan": {"listnet": 1, "listmle": 1}},
    "long": {"cus": 256, "fused_plan": {"hinge": [0, 0], "logistic": [0, 0], "ndcg2": [0, 0]},
            "listwise_plan": {"listnet": 0, "listmle": 0}},
    "bf16-long": {"cus": 256, "fused_plan": {"hinge": [0, 0], "logistic": [0, 0], "ndcg2": [0, 0]},
                 "listwise_plan": {"listnet": 0, "listmle": 0}},
}

EXPECTED = {
    "base": {
        "module-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32"],
        "eager-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "nograd": ["ltr_linear_scores_f32"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
    },
    "base160": {
        "module-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32"],
        "eager-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "nograd": ["ltr_linear_scores_f32"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
    },
    "bf16": {
        "module-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "eager-listnet": ["ltr_linear_scores_bf16", "ltr_listwise_softmax_f32", "ltr_linear_grad_bf16"],
        "nograd": ["ltr_linear_scores_bf16"],
        "step-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32", "ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
    },
    "bf16-160": {
        "module-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "eager-listnet": ["ltr_linear_scores_bf16", "ltr_listwise_softmax_f32", "ltr_linear_grad_bf16"],
        "nograd": ["ltr_linear_scores_bf16"],
        "step-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32", "ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
    },
    "fp16": {
        "module-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["torch", "raises RuntimeError"],
        "lazy-logistic": ["torch", "raises RuntimeError"],
        "lazy-listnet": ["torch", "raises RuntimeError"],
        "eager-hinge": ["torch", "raises RuntimeError"],
        "eager-listnet": ["torch", "raises RuntimeError"],
        "nograd": ["torch", "raises RuntimeError"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-long": ["torch", "raises RuntimeError"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["torch", "raises RuntimeError"],
    },
    "fp64": {
        "module-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["torch", "raises RuntimeError"],
        "lazy-logistic": ["torch", "raises RuntimeError"],
        "lazy-listnet": ["torch", "raises RuntimeError"],
        "eager-hinge": ["torch", "raises RuntimeError"],
        "eager-listnet": ["torch", "raises RuntimeError"],
        "nograd": ["torch", "raises RuntimeError"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-long": ["torch", "raises RuntimeError"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["torch", "raises RuntimeError"],
    },
    "F5": {
        "module-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "module-listmle": ["ltr_linear_scores_f32", "ltr_listmle_f32", "ltr_linear_grad_f32"],
        "module-hinge+scores": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "eager-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32"],
        "eager-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "nograd": ["ltr_linear_scores_f32"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "step-listmle": ["ltr_linear_scores_f32", "ltr_listmle_f32", "ltr_linear_grad_f32"],
        "module-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
    },
    "F46": {
        "module-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "module-listmle": ["ltr_linear_scores_f32", "ltr_listmle_f32", "ltr_linear_grad_f32"],
        "module-hinge+scores": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "eager-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32"],
        "eager-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "nograd": ["ltr_linear_scores_f32"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "step-listmle": ["ltr_linear_scores_f32", "ltr_listmle_f32", "ltr_linear_grad_f32"],
        "module-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
    },
    "F136": {
        "module-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32"],
        "eager-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "nograd": ["ltr_linear_scores_f32"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
    },
    "bf16-F12": {
        "module-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "eager-listnet": ["ltr_linear_scores_bf16", "ltr_listwise_softmax_f32", "ltr_linear_grad_bf16"],
        "nograd": ["ltr_linear_scores_bf16"],
        "step-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32", "ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
    },
    "ragged4": {
        "module-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32"],
        "eager-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "nograd": ["ltr_linear_scores_f32"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["raises ValueError"],
        "loop": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32", "ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
    },
    "bf16-ragged8": {
        "module-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "eager-listnet": ["ltr_linear_scores_bf16", "ltr_listwise_softmax_f32", "ltr_linear_grad_bf16"],
        "nograd": ["ltr_linear_scores_bf16"],
        "step-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32", "ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
    },
    "strided": {
        "module-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "module-listmle": ["ltr_linear_scores_f32", "ltr_listmle_f32", "ltr_linear_grad_f32"],
        "module-hinge+scores": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32"],
        "lazy-logistic": ["ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32"],
        "lazy-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "eager-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32"],
        "eager-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "nograd": ["ltr_linear_scores_f32"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "step-listmle": ["ltr_linear_scores_f32", "ltr_listmle_f32", "ltr_linear_grad_f32"],
        "module-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32", "ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32"],
    },
    "offset": {
        "module-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "module-listmle": ["ltr_linear_scores_f32", "ltr_listmle_f32", "ltr_linear_grad_f32"],
        "module-hinge+scores": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "eager-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32"],
        "eager-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "nograd": ["ltr_linear_scores_f32"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "step-listmle": ["ltr_linear_scores_f32", "ltr_listmle_f32", "ltr_linear_grad_f32"],
        "module-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "raises RuntimeError"],
        "loop": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32", "ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
    },
    "bf16-offset": {
        "module-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "eager-listnet": ["ltr_linear_scores_bf16", "ltr_listwise_softmax_f32", "ltr_linear_grad_bf16"],
        "nograd": ["ltr_linear_scores_bf16"],
        "step-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32", "ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
    },
    "xgrad": {
        "module-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32"],
        "lazy-logistic": ["ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32"],
        "lazy-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "eager-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32"],
        "eager-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "nograd": ["ltr_linear_scores_f32"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32", "ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32"],
    },
    "autocast": {
        "module-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["torch", "ltr_pairwise_loss_f32"],
        "lazy-logistic": ["torch", "ltr_pairwise_loss_f32"],
        "lazy-listnet": ["torch", "ltr_listwise_softmax_f32"],
        "eager-hinge": ["torch", "ltr_pairwise_loss_f32"],
        "eager-listnet": ["torch", "ltr_listwise_softmax_f32"],
        "nograd": ["torch"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-long": ["torch", "ltr_pairwise_loss_f32"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["torch", "ltr_pairwise_loss_f32", "torch", "ltr_pairwise_loss_f32"],
    },
    "cpu": {
        "module-hinge": ["raises RuntimeError"],
        "module-logistic": ["raises RuntimeError"],
        "module-ndcg2": ["raises RuntimeError"],
        "module-listnet": ["raises RuntimeError"],
        "module-listmle": ["raises RuntimeError"],
        "module-hinge+scores": ["raises RuntimeError"],
        "lazy-hinge": ["torch", "raises RuntimeError"],
        "lazy-logistic": ["torch", "raises RuntimeError"],
        "lazy-listnet": ["torch", "raises RuntimeError"],
        "eager-hinge": ["torch", "raises RuntimeError"],
        "eager-listnet": ["torch", "raises RuntimeError"],
        "nograd": ["torch", "raises RuntimeError"],
        "step-hinge": ["raises RuntimeError"],
        "step-ndcg2": ["raises RuntimeError"],
        "step-listnet": ["raises RuntimeError"],
        "step-listmle": ["raises RuntimeError"],
        "module-long": ["raises RuntimeError"],
        "lazy-long": ["torch", "raises RuntimeError"],
        "step-long": ["raises RuntimeError"],
        "lazysgd": ["raises RuntimeError"],
        "loop": ["torch", "raises RuntimeError"],
    },
    "nobias": {
        "module-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_f32", "ltr_linear_grad_f32"],
        "eager-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "nograd": ["ltr_linear_scores_f32"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["raises ValueError"],
        "loop": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32", "ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
    },
    "B0": {
        "module-hinge": [],
        "module-logistic": [],
        "module-ndcg2": [],
        "module-listnet": ["ltr_linear_grad_f32"],
        "module-listmle": ["ltr_linear_grad_f32"],
        "module-hinge+scores": [],
        "lazy-hinge": [],
        "lazy-logistic": [],
        "lazy-listnet": ["ltr_linear_grad_f32"],
        "eager-hinge": ["ltr_linear_grad_f32"],
        "eager-listnet": ["ltr_linear_grad_f32"],
        "nograd": [],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_grad_f32"],
        "step-listmle": ["ltr_linear_grad_f32"],
        "module-long": [],
        "lazy-long": [],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "raises RuntimeError"],
        "loop": [],
    },
    "wrong-weight": {
        "module-hinge": ["raises ValueError"],
        "module-logistic": ["raises ValueError"],
        "module-ndcg2": ["raises ValueError"],
        "module-listnet": ["raises ValueError"],
        "module-listmle": ["raises ValueError"],
        "module-hinge+scores": ["raises ValueError"],
        "lazy-hinge": ["torch", "raises RuntimeError"],
        "lazy-logistic": ["torch", "raises RuntimeError"],
        "lazy-listnet": ["torch", "raises RuntimeError"],
        "eager-hinge": ["torch", "raises RuntimeError"],
        "eager-listnet": ["torch", "raises RuntimeError"],
        "nograd": ["torch", "raises RuntimeError"],
        "step-hinge": ["raises RuntimeError"],
        "step-ndcg2": ["raises RuntimeError"],
        "step-listnet": ["raises RuntimeError"],
        "step-listmle": ["raises RuntimeError"],
        "module-long": ["raises ValueError"],
        "lazy-long": ["torch", "raises RuntimeError"],
        "step-long": ["raises RuntimeError"],
        "lazysgd": ["raises ValueError"],
        "loop": ["torch", "raises RuntimeError"],
    },
    "few-lists": {
        "module-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "module-logistic": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "module-ndcg2": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "lazy-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "lazy-logistic": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "eager-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "nograd": ["ltr_linear_scores_f32"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "lazy-long": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32", "ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
    },
    "bf16-few-lists": {
        "module-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "eager-listnet": ["ltr_linear_scores_bf16", "ltr_listwise_softmax_f32", "ltr_linear_grad_bf16"],
        "nograd": ["ltr_linear_scores_bf16"],
        "step-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32", "ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
    },
    "bf16-F136-L256": {
        "module-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "eager-listnet": ["ltr_linear_scores_bf16", "ltr_listwise_softmax_f32", "ltr_linear_grad_bf16"],
        "nograd": ["ltr_linear_scores_bf16"],
        "step-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32", "ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
    },
    "bf16-F136-L257": {
        "module-hinge": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "module-logistic": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "module-ndcg2": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "lazy-hinge": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "lazy-logistic": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "eager-listnet": ["ltr_linear_scores_bf16", "ltr_listwise_softmax_f32", "ltr_linear_grad_bf16"],
        "nograd": ["ltr_linear_scores_bf16"],
        "step-hinge": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "step-ndcg2": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "lazy-long": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "step-long": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16", "ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
    },
    "bf16-F704-L80": {
        "module-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "eager-listnet": ["ltr_linear_scores_bf16", "ltr_listwise_softmax_f32", "ltr_linear_grad_bf16"],
        "nograd": ["ltr_linear_scores_bf16"],
        "step-hinge": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_bf16", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_partials_bf16", "ltr_linear_reduce_f32", "ltr_linear_partials_bf16", "ltr_linear_reduce_f32"],
    },
    "bf16-F704-L81": {
        "module-hinge": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "module-logistic": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "module-ndcg2": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "lazy-hinge": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "lazy-logistic": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "eager-listnet": ["ltr_linear_scores_bf16", "ltr_listwise_softmax_f32", "ltr_linear_grad_bf16"],
        "nograd": ["ltr_linear_scores_bf16"],
        "step-hinge": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "step-ndcg2": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "lazy-long": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "step-long": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16", "ltr_linear_scores_bf16", "ltr_pairwise_loss_f32", "ltr_linear_grad_bf16"],
    },
    "B160-L768": {
        "module-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "eager-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "nograd": ["ltr_linear_scores_f32"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
    },
    "B160-L769": {
        "module-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "module-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "eager-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "nograd": ["ltr_linear_scores_f32"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
    },
    "cluster": {
        "module-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "eager-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "nograd": ["ltr_linear_scores_f32"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
    },
    "parts": {
        "module-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "module-logistic": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "module-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "lazy-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "lazy-logistic": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "eager-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "nograd": ["ltr_linear_scores_f32"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "lazy-long": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32", "ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
    },
    "B80-L500-F512": {
        "module-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "module-ndcg2": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "module-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "module-hinge+scores": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-logistic": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_f32"],
        "eager-hinge": ["ltr_linear_scores_f32", "ltr_pairwise_loss_ws_f32", "ltr_linear_grad_f32"],
        "eager-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "nograd": ["ltr_linear_scores_f32"],
        "step-hinge": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-ndcg2": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listnet": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "step-listmle": ["ltr_linear_listwise_partials_f32", "ltr_linear_reduce_loss_f32"],
        "module-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "lazy-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_f32"],
        "step-long": ["ltr_linear_partials_f32", "ltr_linear_reduce_loss_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
        "loop": ["ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"],
    },
    "long": {
        "module-hinge": ["ltr_linear_partials_f32", "raises RuntimeError"],
        "module-logistic": ["ltr_linear_partials_f32", "raises RuntimeError"],
        "module-ndcg2": ["ltr_linear_partials_f32", "raises RuntimeError"],
        "module-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "module-listmle": ["ltr_linear_scores_f32", "ltr_listmle_f32", "ltr_linear_grad_f32"],
        "module-hinge+scores": ["ltr_linear_partials_f32", "raises RuntimeError"],
        "lazy-hinge": ["ltr_linear_partials_f32", "raises RuntimeError"],
        "lazy-logistic": ["ltr_linear_partials_f32", "raises RuntimeError"],
        "lazy-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "eager-hinge": ["ltr_linear_scores_f32", "raises ValueError"],
        "eager-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "nograd": ["ltr_linear_scores_f32"],
        "step-hinge": ["ltr_linear_partials_f32", "raises RuntimeError"],
        "step-ndcg2": ["ltr_linear_partials_f32", "raises RuntimeError"],
        "step-listnet": ["ltr_linear_scores_f32", "ltr_listwise_softmax_f32", "ltr_linear_grad_f32"],
        "step-listmle": ["ltr_linear_scores_f32", "ltr_listmle_f32", "ltr_linear_grad_f32"],
        "module-long": ["ltr_linear_scores_f32", "ltr_pairwise_loss_long_f32", "ltr_linear_grad_f32"],
        "lazy-long": ["ltr_linear_scores_f32", "ltr_pairwise_loss_long_f32", "ltr_linear_grad_f32"],
        "step-long": ["ltr_linear_scores_f32", "ltr_pairwise_loss_long_f32", "ltr_linear_grad_f32"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "raises RuntimeError"],
        "loop": ["ltr_linear_sgd_lazy_step_dp_f32", "raises RuntimeError"],
    },
    "bf16-long": {
        "module-hinge": ["ltr_linear_scores_bf16", "raises ValueError"],
        "module-logistic": ["ltr_linear_scores_bf16", "raises ValueError"],
        "module-ndcg2": ["ltr_linear_scores_bf16", "raises ValueError"],
        "module-listnet": ["ltr_linear_scores_bf16", "ltr_listwise_softmax_f32", "ltr_linear_grad_bf16"],
        "module-listmle": ["ltr_linear_scores_bf16", "ltr_listmle_f32", "ltr_linear_grad_bf16"],
        "module-hinge+scores": ["ltr_linear_scores_bf16", "raises ValueError"],
        "lazy-hinge": ["ltr_linear_scores_bf16", "raises ValueError"],
        "lazy-logistic": ["ltr_linear_scores_bf16", "raises ValueError"],
        "lazy-listnet": ["ltr_linear_scores_bf16", "ltr_listwise_softmax_f32", "ltr_linear_grad_bf16"],
        "eager-hinge": ["ltr_linear_scores_bf16", "raises ValueError"],
        "eager-listnet": ["ltr_linear_scores_bf16", "ltr_listwise_softmax_f32", "ltr_linear_grad_bf16"],
        "nograd": ["ltr_linear_scores_bf16"],
        "step-hinge": ["ltr_linear_scores_bf16", "raises ValueError"],
        "step-ndcg2": ["ltr_linear_scores_bf16", "raises ValueError"],
        "step-listnet": ["ltr_linear_scores_bf16", "ltr_listwise_softmax_f32", "ltr_linear_grad_bf16"],
        "step-listmle": ["ltr_linear_scores_bf16", "ltr_listmle_f32", "ltr_linear_grad_bf16"],
        "module-long": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_long_f32", "ltr_linear_grad_bf16"],
        "lazy-long": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_long_f32", "ltr_linear_grad_bf16"],
        "step-long": ["ltr_linear_scores_bf16", "ltr_pairwise_loss_long_f32", "ltr_linear_grad_bf16"],
        "lazysgd": ["ltr_linear_sgd_lazy_step_dp_f32", "raises RuntimeError"],
        "loop": ["ltr_linear_scores_bf16", "raises ValueError"],
    },
}


# ---- what a route means, per caller: the entry points in call order ----
P32, P16, PLW = "ltr_linear_partials_f32", "ltr_linear_partials_bf16", "ltr_linear_listwise_partials_f32"
REDUCE, REDUCE_LOSS = "ltr_linear_reduce_f32", "ltr_linear_reduce_loss_f32"
LAZY_STEP, FLUSH = "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32"


def _kind(fused, loss, long_lists):
    from pytorchltr_amd._autograd import LongKind
    kind = fused._resolve_loss(loss)[0]
    return LongKind(kind) if long_lists else kind


def _data16(case):
    """`fused._bf16_batch`: a bf16 batch on the device that needs no gradient itself, outside autocast."""
    return case["dtype"] == "bfloat16" and not (case["cpu"] or case["xgrad"] or case["autocast"])


def _loss_entry(fused, case, loss, long_lists):
    """The stand-alone loss on computed scores: its entry point, or how it declines the list length."""
    if loss in ("listnet", "listmle"):
        return {"listnet": "ltr_listwise_softmax_f32", "listmle": "ltr_listmle_f32"}[loss]
    if case["L"] > MAX_LIST_LEN:
        return "ltr_pairwise_loss_long_f32" if long_lists else "raises ValueError"
    split = fused._C.lib().ltr_pairwise_loss_workspace_bytes(fused._resolve_loss(loss)[0], case["B"], case["L"]) != 0
    return "ltr_pairwise_loss_ws_f32" if split else "ltr_pairwise_loss_f32"


def _pieces(fused, case, loss, long_lists, family):
    """Scorer, stand-alone loss, weight gradient; an empty batch launches the gradient's zero-fill alone."""
    if case["B"] == 0:
        return [family.grad]
    entry = _loss_entry(fused, case, loss, long_lists)
    return [family.scores, entry] + ([] if entry.startswith("raises") else [family.grad])


def _scorer(case, lazy, grad=True):
    """What LinearScorer.forward hands back: "torch" (F.linear), "lazy" (LazyScores) or "scores" (computed at once)."""
    if case["cpu"] or case["autocast"] or case["wrong_weight"] or not (case["dtype"] == "float32" or _data16(case)):
        return "torch"
    return "lazy" if lazy and grad and not case["xgrad"] and case["view"] != "strided" else "scores"


def _torch_layer(fused, case, loss, long_lists):
    """F.linear, then the stand-alone loss on its scores (autograd's own backward); a batch it does not take raises."""
    if case["cpu"] or case["wrong_weight"] or case["dtype"] in ("float16", "float64"):
        return ["torch", "raises RuntimeError"]
    return ["torch"] + ([_loss_entry(fused, case, loss, long_lists)] if loss else [])


def _route(fused, what, case, loss, long_lists, ans):
    """`fused._linear_route` on the case's plain values and the library's recorded answers."""
    F, ragged = case["F"], case["view"] == "ragged"
    listwise = loss in ("listnet", "listmle")
    aligned = not (case["view"] == "offset" and case["dtype"] == "float32")     # (another dtype is cast: a new tensor)
    # the asymmetry of DESIGN 24: FusedLinearLoss asks the pieces rule with in_features, LazyScores with F4 on a view
    Fq = f4(F) if what == "lazy" and ragged else F
    return fused._linear_route(
        what, getattr(torch, case["dtype"]), 3, not case["cpu"], case["xgrad"], case["autocast"],
        _kind(fused, loss, long_lists), case["B"], case["L"], rows_in_memory(case) if listwise else F, ans["cus"], Fq,
        False, None if listwise else ans["fused_plan"][loss][Fq != F],
        bool(listwise and ans["listwise_plan"][loss] and aligned))


def _routed(fused, what, case, loss, long_lists, ans):
    """The entry points of the route that `_linear_route` names for a caller that asks it."""
    if case["cpu"]:
        return ["raises RuntimeError"]                  # (the prepare step, in front of every route)
    if case["wrong_weight"] and what != "lazy":         # (the weight-count checks; a LinearScorer is the torch layer there)
        return ["raises ValueError" if what == "module" else "raises RuntimeError"]
    route = _route(fused, what, case, loss, long_lists, ans)
    assert route != fused._LIN_SCORES
    if route in fused._LIN_PIECES:
        return _pieces(fused, case, loss, long_lists, fused._LINEAR_BF16 if route == fused._LIN_BF16_PIECES else fused._LINEAR_F32)
    entry = {fused._LIN_F32: P32, fused._LIN_BF16_FUSED: P16, fused._LIN_LISTWISE: PLW}[route]
    if what == "step":                                  # (hands an empty batch to the entry points)
        return [entry, "raises RuntimeError" if case["L"] > MAX_LIST_LEN else REDUCE_LOSS]
    if case["B"] == 0:
        return []                                       # (the autograd function launches nothing)
    return [entry, "raises RuntimeError" if case["L"] > MAX_LIST_LEN else REDUCE]


def _lazy_launch(case):
    """Where `_LinearLossFunction` takes the lazy launch on a fused fp32 pairwise route (its own conditions and
    `_LazyLinear.forward`'s): a bias, rows as wide in memory as the weight, 16-byte aligned, a batch that is not empty."""
    return (case["bias"] and rows_in_memory(case) == case["F"] and case["view"] != "offset" and case["B"] > 0
            and case["dtype"] == "float32")


def _twice(seq):
    return seq if seq and seq[-1].startswith("raises") else seq + seq


def _predicted(fused, caller, case, ans):
    what, loss = CALLERS[caller]
    long_lists = what.endswith("-long")
    what = what[:-5] if long_lists else what
    if what in ("module", "step"):
        return _routed(fused, what, case, loss, long_lists, ans)
    if what == "lazysgd":                               # asks no route: fp32 always, its own checks, the C ABI's
        if case["cpu"]:
            return ["raises RuntimeError"]
        if not case["bias"] or case["wrong_weight"] or rows_in_memory(case) != case["F"]:
            return ["raises ValueError"]
        unaligned = case["view"] == "offset" and case["dtype"] == "float32"
        if case["L"] > MAX_LIST_LEN or case["B"] == 0 or unaligned:
            return [LAZY_STEP, "raises RuntimeError"]
        return [LAZY_STEP, LAZY_STEP, FLUSH]
    scorer = _scorer(case, lazy=what in ("lazy", "loop"), grad=what != "nograd")
    family = fused._LINEAR_BF16 if _data16(case) else fused._LINEAR_F32
    if what == "nograd":
        return _torch_layer(fused, case, None, False) if scorer == "torch" else [family.scores] if case["B"] else []
    if scorer == "torch":
        once = _torch_layer(fused, case, loss, long_lists)
    elif scorer == "scores":
        once = _pieces(fused, case, loss, long_lists, family)
    else:
        once = _routed(fused, "lazy", case, loss, long_lists, ans)
        if what == "loop" and once[:1] == [P32] and _lazy_launch(case):
            return [LAZY_STEP, "raises RuntimeError"] if case["L"] > MAX_LIST_LEN else [LAZY_STEP, LAZY_STEP, FLUSH]
    return _twice(once) if what == "loop" else once


@pytest.fixture(scope="module")
def fused():
    from pytorchltr_amd import _C, fused
    from pytorchltr_amd.build import build_extension
    import os
    if not os.environ.get("LTR_HIP_LIB"):
        build_extension()
    assert _C.max_list_len() == MAX_LIST_LEN
    return fused


def test_the_tables_cover_every_case_and_caller():
    assert sorted(EXPECTED) == sorted(ANSWERS) == sorted(CASES)
    for name in CASES:
        assert list(EXPECTED[name]) == list(CALLERS), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_route_function_states_the_recorded_table(fused, name):
    for caller in CALLERS:
        assert _predicted(fused, caller, CASES[name], ANSWERS[name]) == EXPECTED[name][caller], caller


def test_the_recorded_table_shows_every_route(fused):
    """Every named route but _LIN_SCORES (LazyScores whose scores exist: no entry point of its own) is some case's."""
    seen = set()
    for name, case in CASES.items():
        for caller, (what, loss) in CALLERS.items():
            long_lists = what.endswith("-long")
            what = what[:-5] if long_lists else what
            if what in ("module", "step", "lazy") and not case["cpu"]:
                seen.add(_route(fused, what, case, loss, long_lists, ANSWERS[name]))
    assert seen == {fused._LIN_F32, fused._LIN_BF16_FUSED, fused._LIN_LISTWISE, fused._LIN_F32_PIECES, fused._LIN_BF16_PIECES}
    assert fused._linear_route("lazy", torch.float32, 3, True, False, False, 0, 2, 5, 8, 256, computed=True) == fused._LIN_SCORES
    assert fused._linear_route("lazy", torch.float32, 3, True, False, False, fused._LISTWISE_SOFTMAX, 2, 5, 8, 256) \
        == fused._LIN_SCORES


def test_the_callers_hold_no_route_logic_of_their_own(fused, monkeypatch):
    """With `_linear_routed` answering each route in turn, each caller performs that route's action -- whatever the batch
    is: the fused function, the pieces, or (LazyScores) None -- and asks nothing else."""
    done = []
    xs = torch.zeros(2, 5, 8)
    y, n = torch.zeros(2, 5, dtype=torch.int64), torch.tensor([5, 3])

    class Apply:
        def __init__(self, name):
            self.name = name

        def apply(self, *args):
            done.append(self.name)
            return torch.zeros(2, 5, 1) if self.name == "scores" else torch.zeros(2)

    monkeypatch.setattr(fused, "_LinearLossFunction", Apply("fused"))
    monkeypatch.setattr(fused, "_LinearScoreFunction", Apply("scores"))
    monkeypatch.setattr(fused, "_loss_pieces", lambda *a: (done.append("loss"), torch.zeros(2))[1])
    monkeypatch.setattr(fused, "_step_pieces", lambda *a: (done.append("step pieces"), None)[1])
    class Reached(Exception):
        pass

    def prepare(*args, **kwargs):
        raise Reached

    monkeypatch.setattr(fused, "_linear_prepare", prepare)
    for name in ("_prefer_pieces", "_long_pair_shape", "_listwise_fused", "_linear_bf16_plan", "_linear_route", "_bf16_batch"):
        monkeypatch.setattr(fused, name, lambda *a, **kw: pytest.fail("a caller asked %s itself" % name))
    module = fused.FusedLinearLoss(8, "hinge")
    scorer = fused.LinearScorer(8)
    for route in (fused._LIN_F32, fused._LIN_BF16_FUSED, fused._LIN_LISTWISE, fused._LIN_F32_PIECES, fused._LIN_BF16_PIECES,
                  fused._LIN_SCORES):
        monkeypatch.setattr(fused, "_linear_routed", lambda *a, **kw: (route, xs))
        pieces, is_fused = route in fused._LIN_PIECES, route not in fused._LIN_PIECES + (fused._LIN_SCORES,)
        del done[:]
        module(xs, y, n)
        assert done == (["scores", "loss"] if pieces else ["fused"]), route
        del done[:]
        out = fused.LazyScores(xs, scorer.weight, scorer.bias, n).fused_loss(y, n, 0, 1.0)
        assert (done, out is None) == ((["fused"], False) if is_fused else ([], True)), route
        del done[:]
        if pieces:
            fused.linear_loss_step(xs, scorer.weight, scorer.bias, y, n)
            assert done == ["step pieces"], route
        elif is_fused:
            with pytest.raises(Reached):                # (the prepare step of the fused launch: reached, and nothing before it)
                fused.linear_loss_step(xs, scorer.weight, scorer.bias, y, n)
            assert done == [], route
