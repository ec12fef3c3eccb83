"""Listwise losses on MI355X: softmax cross-entropy (ListNet top-one) and ListMLE (the Plackett-Luce likelihood).

NOT part of the reference: ``pytorchltr/loss/__init__.py:1-7`` exports the seven pairwise classes
only and nothing in the reference's code, tests or docs defines a listwise loss.  The project
brief names "listwise softmax cross-entropy" on the hot path, so this module provides it with the
same call signature as the reference's losses -- **parity unpinned: there is no reference
implementation to pin it to**; the specification is ``include/ltr_hip.h``
(``ltr_listwise_softmax_f32``), restated in fp64 by ``oracle/ltr_oracle.c`` and checked against
finite differences.
"""
import torch as _torch
from torch.autograd.function import once_differentiable as _once

from pytorchltr_amd import _C
from pytorchltr_amd import _ties
from pytorchltr_amd._prepare import prepare as _prepare


def _fused_step(scores, relevance, n, loss, k, sigma=1.0):
    """Scores a LinearScorer has not computed yet (fused.LazyScores) are asked for the fused Linear step first --
    scorer, loss and weight-gradient rows in one launch, no score matrix written: (loss[b], None).  Where that step does
    not apply (ltr_linear_listwise_plan declines the shape, the scores were computed already) they are computed here,
    autograd-connected to the layer: (None, scores), as for any other scores."""
    fused = getattr(scores, "fused_loss", None)
    if fused is None:
        return None, scores
    from pytorchltr_amd.fused import _ListwiseKind
    out = fused(relevance, n, _ListwiseKind(loss, k), sigma)           # (sigma: LambdaRankLoss, loss/pairwise_lambda.py)
    return (None, scores.materialize()) if out is None else (out, None)


class _ListwiseSoftmaxFunction(_torch.autograd.Function):
    """Its own small Function: the pairwise plumbing does not apply -- the kernel has no
    LDS-bound list limit (one wave walks the list), and it computes in fp32 whatever the score dtype
    (fp64 / half scores are cast in and the result cast back, gradients included)."""

    @staticmethod
    def forward(ctx, scores, relevance, n):
        s, r, nn = _prepare(scores, relevance, n, allow_f64=False, limit_len=False)
        B, L = s.shape
        need_grad = ctx.needs_input_grad[0]
        loss = _torch.empty(B, dtype=_torch.float32, device=s.device)
        ds = _torch.empty(B, L, dtype=_torch.float32, device=s.device) if need_grad else None
        if B > 0:
            with _C.device_ctx(s):
                _C.check(_C.lib().ltr_listwise_softmax_f32(_C.ptr(s), _C.ptr(r), _C.label_dtype(r), _C.ptr(nn), B, L,
                                                           _C.ptr(loss), _C.ptr(ds), _C.stream_of(s)))
        if need_grad:
            ctx.save_for_backward(ds)
        ctx.in_shape, ctx.in_dtype = scores.shape, scores.dtype
        return loss if scores.dtype is _torch.float32 else loss.to(scores.dtype)

    @staticmethod
    @_once
    def backward(ctx, grad_out):
        (ds,) = ctx.saved_tensors
        out = ds * grad_out.reshape(-1, 1).to(ds.dtype)
        return out.reshape(ctx.in_shape).to(ctx.in_dtype), None, None


class ListwiseSoftmaxLoss(_torch.nn.Module):
    r"""ListNet top-one cross-entropy between the label and the score distributions of a query:

    .. math::
        l(\mathbf{s}, \mathbf{y}) = -\sum_{j < n} \mathrm{softmax}(\mathbf{y})_j
        \ln \mathrm{softmax}(\mathbf{s})_j

    over the ``n`` real documents (padded documents take no part); ``n = 0`` gives 0.

    Shape:
        - scores: :math:`(N, \texttt{list\_size})` or :math:`(N, \texttt{list\_size}, 1)`
        - relevance: :math:`(N, \texttt{list\_size})`
        - n: :math:`(N)`
        - output: :math:`(N)`
    """

    def __init__(self):
        super().__init__()

    def forward(self, scores: _torch.FloatTensor, relevance: _torch.LongTensor,
                n: _torch.LongTensor) -> _torch.FloatTensor:
        out, scores = _fused_step(scores, relevance, n, _C.LISTWISE_LISTNET, None)
        return out if out is not None else _ListwiseSoftmaxFunction.apply(scores, relevance, n)


ListNetLoss = ListwiseSoftmaxLoss


class _ListMLEFunction(_torch.autograd.Function):
    """ltr_listmle_f32 (include/ltr_listwise.h): loss and d loss / d scores in one forward; backward is a row scale.
    Computes in fp32 whatever the score dtype, like _ListwiseSoftmaxFunction."""

    @staticmethod
    def forward(ctx, scores, relevance, n, k):
        s, r, nn = _prepare(scores, relevance, n, allow_f64=False, limit_len=False)
        B, L = s.shape
        if L > _C.max_sort_list_len():
            raise ValueError("list_size %d exceeds the supported maximum %d" % (L, _C.max_sort_list_len()))
        need_grad = ctx.needs_input_grad[0]
        loss = _torch.empty(B, dtype=_torch.float32, device=s.device)
        ds = _torch.empty(B, L, dtype=_torch.float32, device=s.device) if need_grad else None
        if B > 0:
            lib = _C.lib()
            sd = _ties.draw_seed(L, s.device)
            # (0 bytes: one workgroup per query, no workspace)
            ws, nbytes = _C.workspace(lib.ltr_listmle_workspace_bytes(B, L), s.device)
            with _C.device_ctx(s):
                _C.check(lib.ltr_listmle_f32(
                    _C.ptr(s), _C.ptr(r), _C.label_dtype(r), _C.ptr(nn), int(k or 0), *_ties.tie_args(sd), B, L,
                    _C.ptr(loss), _C.ptr(ds), _C.ptr(ws), nbytes, _C.stream_of(s)))
        if need_grad:
            ctx.save_for_backward(ds)
        ctx.in_shape, ctx.in_dtype = scores.shape, scores.dtype
        return loss if scores.dtype is _torch.float32 else loss.to(scores.dtype)

    @staticmethod
    @_once
    def backward(ctx, grad_out):
        (ds,) = ctx.saved_tensors
        out = ds * grad_out.reshape(-1, 1).to(ds.dtype)
        return out.reshape(ctx.in_shape).to(ctx.in_dtype), None, None, None


class ListMLELoss(_torch.nn.Module):
    r"""ListMLE (Xia et al. 2008): the negative log-likelihood of the label ordering under a Plackett-Luce model of
    the scores; with ``k``, top-k ListMLE (Xia et al. 2009), the first ``k`` factors of the likelihood only.

    With :math:`\pi` the real documents (:math:`j < n`) ordered by label, descending, and
    :math:`K = \min(k, n)` (:math:`K = n` without ``k``):

    .. math::
        l(\mathbf{s}, \mathbf{y}) = \sum_{m < K} \Big( \ln \sum_{i = m}^{n - 1} e^{s_{\pi(i)}} - s_{\pi(m)} \Big)

    Padded documents take no part; ``n <= 1`` gives 0.  Equal labels are ordered by the tie-breaking mode of
    :mod:`pytorchltr_amd.utils` (``tie_breaking``): one random order per call by default, document index in mode
    ``"index"``.  Any list length up to ``ltr_max_sort_list_len()``; fp16, bf16 and fp64 scores are computed in fp32.

    Shape:
        - scores: :math:`(N, \texttt{list\_size})` or :math:`(N, \texttt{list\_size}, 1)`
        - relevance: :math:`(N, \texttt{list\_size})`
        - n: :math:`(N)`
        - output: :math:`(N)`
    """

    def __init__(self, k=None):
        super().__init__()
        if k is not None:
            if isinstance(k, bool) or int(k) != k or k < 1:
                raise ValueError("k must be a positive integer or None, got %r" % (k,))
            k = int(k)
        self.k = k

    def forward(self, scores: _torch.FloatTensor, relevance: _torch.LongTensor,
                n: _torch.LongTensor) -> _torch.FloatTensor:
        out, scores = _fused_step(scores, relevance, n, _C.LISTWISE_LISTMLE, self.k)
        return out if out is not None else _ListMLEFunction.apply(scores, relevance, n, self.k)

    def extra_repr(self):
        return "" if self.k is None else "k=%d" % self.k
