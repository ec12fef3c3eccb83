"""Ranking metrics and the pytrec_eval export: the names pytorchltr/evaluation/__init__.py:1-4
exports, same signatures; and evaluate(), many metrics from one ranking pass on the GPU."""
from pytorchltr_amd.evaluation.arp import arp
from pytorchltr_amd.evaluation.dcg import dcg, ndcg
from pytorchltr_amd.evaluation.metrics import (average_precision, err, evaluate, precision, recall,
                                               reciprocal_rank)
from pytorchltr_amd.evaluation.trec import generate_pytrec_eval

__all__ = ["arp", "dcg", "ndcg", "generate_pytrec_eval", "evaluate", "average_precision", "reciprocal_rank",
           "precision", "recall", "err"]
