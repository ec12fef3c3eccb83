"""LambdaLoss family on MI355X.

API parity with the reference's loss/pairwise_lambda.py.  The reference sorts by score,
gathers scores and labels into rank order and evaluates a weighted log-sigmoid on every
(rank i, rank j) pair (:67-89).  Here the rank of every document is obtained by an in-LDS
counting rank and the pair weights are evaluated in document order inside one fused kernel;
the ranking is a constant w.r.t. autograd in both implementations.

Tie rule (documented deviation): score ties are broken by document index, not by the
reference's global-RNG permutation (utils/tensor_operations.py:43-45).
"""
import torch as _torch
from torch.autograd.function import once_differentiable as _once

from pytorchltr_amd import _C
from pytorchltr_amd._autograd import pairwise_loss as _pairwise_loss
from pytorchltr_amd._prepare import prepare as _prepare


class LambdaLoss(_torch.nn.Module):
    """LambdaLoss base (reference :6-92)."""
    _kind = None

    def __init__(self, sigma: float = 1.0, *, long_lists: bool = False):
        """
        Args:
            sigma: Steepness of the logistic curve.
            long_lists: Take lists of more than ``_C.max_list_len()`` = 4096 documents, up to
                ``_C.max_pair_list_len()`` = 65 536 (``ltr_pairwise_loss_long_f32``; the reference has no such
                bound).  The work is quadratic in the list length, so the default keeps raising ``ValueError``.
        """
        super().__init__()
        self.sigma = sigma
        self.long_lists = bool(long_lists)

    def forward(self, scores: _torch.FloatTensor, relevance: _torch.LongTensor,
                n: _torch.LongTensor) -> _torch.FloatTensor:
        """Per-query loss; arguments as for the additive losses."""
        if self._kind is None:
            raise NotImplementedError
        return _pairwise_loss(scores, relevance, n, self._kind, self.sigma, self.long_lists)


class LambdaARPLoss1(LambdaLoss):
    r"""ARP Loss 1 (reference :95-117):
    :math:`-\sum_{i,j} \log_2 \mathrm{sigmoid}(\sigma (s_{\pi_i} - s_{\pi_j}))^{y_{\pi_i}}`."""
    _kind = _C.ARP1


class LambdaARPLoss2(LambdaLoss):
    r"""ARP Loss 2 (reference :120-140):
    :math:`\sum_{y_i > y_j} |y_i - y_j| \log_2(1 + e^{-\sigma (s_i - s_j)})`."""
    _kind = _C.ARP2


class LambdaNDCGLoss1(LambdaLoss):
    r"""NDCG Loss 1 (reference :143-173): exponent :math:`G_{\pi_i} / D_i` with
    :math:`G = (2^y - 1) / \mathrm{maxDCG}` and :math:`D_i = \log_2(2 + i)` (0-based rank).

    Negative integer grades take the float formula :math:`2^y - 1` (a grade of -1 has the gain -0.5, whatever the label
    dtype); the reference computes ``2 ** y`` on the integer tensor, where ``2 ** -1 == 0`` and the gain is -1.  Float
    labels of the same values agree with the reference."""
    _kind = _C.NDCG1


class LambdaNDCGLoss2(LambdaLoss):
    r"""NDCG Loss 2 (reference :176-218): exponent :math:`\delta_{ij} |G_{\pi_i} - G_{\pi_j}|`
    over pairs with :math:`y_i > y_j`, :math:`\delta_{ij} = |1/D_{|i-j|} - 1/D_{|i-j|+1}|`,
    :math:`D_k = \log_2(2 + k)` as the reference code (not its docstring) has it.

    Negative integer grades take the float formula :math:`2^y - 1` (a grade of -1 has the gain -0.5, whatever the label
    dtype); the reference computes ``2 ** y`` on the integer tensor, where ``2 ** -1 == 0`` and the gain is -1.  Float
    labels of the same values agree with the reference."""
    _kind = _C.NDCG2


class _LambdaRankFunction(_torch.autograd.Function):
    """ltr_lambdarank_f32 (include/ltr_lambdarank.h), and past max_list_len() documents ltr_lambdarank_long_f32
    (include/ltr_lambdarank_long.h): loss and d loss / d scores in one forward; backward is a row scale.  Computes in
    fp32 whatever the score dtype (fp64 / half scores are cast in and the result cast back, gradients included)."""

    @staticmethod
    def forward(ctx, scores, relevance, n, k, sigma):
        s, r, nn = _prepare(scores, relevance, n, allow_f64=False, limit_len=False)
        B, L = s.shape
        if L > _C.max_pair_list_len():
            raise ValueError("list_size %d exceeds max_pair_list_len() = %d, the bound of LambdaRankLoss (ListMLELoss and "
                             "ListwiseSoftmaxLoss take longer lists)" % (L, _C.max_pair_list_len()))
        need_grad = ctx.needs_input_grad[0]
        loss = _torch.empty(B, dtype=_torch.float32, device=s.device)
        ds = _torch.empty(B, L, dtype=_torch.float32, device=s.device) if need_grad else None
        if B > 0:
            lib = _C.lib()
            kk = min(int(k or 0), 0x7FFFFFFF)
            with _C.device_ctx(s):
                if L > _C.max_list_len():
                    # past one workgroup's LDS: everything by rank in a workspace, owner tiles against the streamed anchors
                    ws, ws_bytes = _C.workspace(lib.ltr_lambdarank_long_workspace_bytes(kk, B, L), s.device)
                    _C.check(lib.ltr_lambdarank_long_f32(_C.ptr(s), _C.ptr(r), _C.label_dtype(r), _C.ptr(nn), kk,
                                                         float(sigma), B, L, _C.ptr(loss), _C.ptr(ds), _C.ptr(ws), ws_bytes,
                                                         _C.stream_of(s)))
                else:
                    _C.check(lib.ltr_lambdarank_f32(_C.ptr(s), _C.ptr(r), _C.label_dtype(r), _C.ptr(nn), kk,
                                                    float(sigma), B, L, _C.ptr(loss), _C.ptr(ds), _C.stream_of(s)))
        if need_grad:
            ctx.save_for_backward(ds)
        ctx.in_shape, ctx.in_dtype = scores.shape, scores.dtype
        return loss if scores.dtype is _torch.float32 else loss.to(scores.dtype)

    @staticmethod
    @_once
    def backward(ctx, grad_out):
        (ds,) = ctx.saved_tensors
        out = ds * grad_out.reshape(-1, 1).to(ds.dtype)
        return out.reshape(ctx.in_shape).to(ctx.in_dtype), None, None, None, None


class LambdaRankLoss(_torch.nn.Module):
    r"""LambdaRank (Burges et al. 2006; the objective of LambdaMART): the pairwise logistic loss with every pair
    weighted by the change in NDCG@k when its two documents swap ranks.

    With :math:`r_j` the 0-based rank of document :math:`j` by score (equal scores by document index, as for the other
    Lambda losses), :math:`K = \min(k, n)` (:math:`K = n` without ``k``), :math:`d(r) = 1 / \log_2(2 + r)` for
    :math:`r < K` and 0 from :math:`K` on, and :math:`G_j = (2^{y_j} - 1) / \mathrm{maxDCG@}K`:

    .. math::
        l(\mathbf{s}, \mathbf{y}) = \sum_{y_i > y_j} |G_i - G_j| \, |d(r_i) - d(r_j)| \,
        \log_2(1 + e^{-\sigma (s_i - s_j)})

    The ranking and the weights are constants of the gradient.  A pair with both documents below the cutoff has weight
    0 and is never visited: the kernel evaluates about :math:`K n` pairs, not :math:`n^2 / 2`.  Padded documents take
    no part; ``n <= 1`` gives 0; a query without a positive gain has maxDCG 1.  Negative grades take the float formula
    :math:`2^y - 1`, as in :class:`LambdaNDCGLoss1`.  fp16, bf16 and fp64 scores are computed in fp32.  The module has
    no parameters (an empty ``state_dict``).

    Lists of up to ``max_pair_list_len()`` = 65 536 documents.  Up to ``max_list_len()`` = 4096 a query is one
    workgroup (``ltr_lambdarank_f32``); longer lists take ``ltr_lambdarank_long_f32`` by themselves, there is no flag to
    set: with a cutoff the work stays about :math:`K n` (two passes over the anchors' pairs with the tail, behind two
    sorts of the list).  **Without a cutoff, or with a very large one, the work past 4096 documents is quadratic**,
    :math:`n^2` pair evaluations per query -- 4.3e9 at the bound -- as for the pairwise losses with
    ``long_lists=True``.

    Shape:
        - scores: :math:`(N, \texttt{list\_size})` or :math:`(N, \texttt{list\_size}, 1)`
        - relevance: :math:`(N, \texttt{list\_size})`
        - n: :math:`(N)`
        - output: :math:`(N)`
    """

    def __init__(self, sigma: float = 1.0, k=None):
        super().__init__()
        if k is not None:
            if isinstance(k, bool) or int(k) != k or k < 1:
                raise ValueError("k must be a positive integer or None, got %r" % (k,))
            k = int(k)
        self.sigma = sigma
        self.k = k

    def forward(self, scores: _torch.FloatTensor, relevance: _torch.LongTensor,
                n: _torch.LongTensor) -> _torch.FloatTensor:
        from pytorchltr_amd.loss.listwise import _fused_step
        out, scores = _fused_step(scores, relevance, n, _C.LISTWISE_LAMBDARANK, self.k, self.sigma)
        return out if out is not None else _LambdaRankFunction.apply(scores, relevance, n, self.k, self.sigma)

    def extra_repr(self):
        return "sigma=%s, k=%s" % (self.sigma, self.k)
