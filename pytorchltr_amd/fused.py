"""Linear scorer fused with a ranking loss (one HIP launch for scores, loss and weight grads).

The reference has no such module: its users write
``loss_fn(torch.nn.Linear(F, 1)(xs), ys, n)`` (examples/01-basic-usage.py:66-75,
tests/test_integration.py:42).  ``FusedLinearLoss`` is that exact composition -- same
parameters (``weight`` (1, F), ``bias`` (1,), state_dict-compatible with ``nn.Linear(F, 1)``),
same per-query output -- computed by ``ltr_linear_partials_f32`` so the (B, L, F) feature
tensor crosses HBM once instead of twice plus the score round trip.
"""
import collections
import ctypes
import math

import torch
from torch.autograd.function import once_differentiable

from . import _C
from ._prepare import prepare_n, prepare_relevance

_KIND_BY_NAME = {
    "hinge": _C.HINGE, "dcg_hinge": _C.DCG_HINGE, "logistic": _C.LOGISTIC,
    "arp1": _C.ARP1, "arp2": _C.ARP2, "ndcg1": _C.NDCG1, "ndcg2": _C.NDCG2,
}


class _ListwiseKind(collections.namedtuple("_ListwiseKind", "loss k", defaults=(None,))):
    """A listwise loss where the pairwise ones are an ``enum ltr_loss_kind`` value: the loss code of
    ``include/ltr_listwise.h`` (ListNet, ListMLE) and ListMLE's ``k`` -- or ``_C.LISTWISE_LAMBDARANK`` with LambdaRank's
    cutoff ``k`` (include/ltr_lambdarank.h: a loss of the same fused Linear step; its sigma travels beside the kind)."""
    __slots__ = ()


_LISTWISE_BY_NAME = {"softmax": _C.LISTWISE_LISTNET, "listnet": _C.LISTWISE_LISTNET, "listmle": _C.LISTWISE_LISTMLE,
                     "lambdarank": _C.LISTWISE_LAMBDARANK}


def _resolve_loss(loss):
    """Accepts a kind name or an instance of a pytorchltr_amd loss module: (kind, sigma); a listwise loss ("softmax" /
    "listnet" / "listmle", ListwiseSoftmaxLoss, ListMLELoss(k)) and LambdaRank ("lambdarank", LambdaRankLoss(sigma, k):
    the loss slot of the listwise step) resolve to a :class:`_ListwiseKind`; a pairwise module
    built with ``long_lists=True`` to a :class:`_autograd.LongKind` (the same int, and the flag with it)."""
    if isinstance(loss, str):
        if loss in _LISTWISE_BY_NAME:
            return _ListwiseKind(_LISTWISE_BY_NAME[loss]), 1.0
        return _KIND_BY_NAME[loss], 1.0
    from .loss import listwise as _lw
    from .loss import pairwise_lambda as _pl
    if isinstance(loss, _pl.LambdaRankLoss):
        return _ListwiseKind(_C.LISTWISE_LAMBDARANK, loss.k), float(loss.sigma)
    if isinstance(loss, _lw.ListMLELoss):
        return _ListwiseKind(_C.LISTWISE_LISTMLE, loss.k), 1.0
    if isinstance(loss, _lw.ListwiseSoftmaxLoss):
        return _ListwiseKind(_C.LISTWISE_LISTNET), 1.0
    kind = getattr(loss, "_kind", None)
    if kind is None:
        raise TypeError("loss must be a kind name or a pytorchltr_amd.loss module")
    if getattr(loss, "long_lists", False):
        from ._autograd import LongKind
        kind = LongKind(kind)
    return kind, float(getattr(loss, "sigma", 1.0))


def _long_pair_shape(kind, L):
    """True for a pairwise kind that opted into long lists (long_lists=True) on a list past max_list_len(): no fused
    kernel holds such a query; the scorer, ltr_pairwise_loss_long_f32 and the streaming weight-gradient kernel do."""
    return getattr(kind, "long_lists", False) and L > _C.max_list_len()


def _pairwise_pieces(scores, relevance, n, kind, sigma):
    """The stand-alone pairwise loss on computed scores (autograd-connected to them)."""
    from ._autograd import PairwiseLossFunction
    return PairwiseLossFunction.apply(scores, relevance, n, int(kind), sigma, bool(getattr(kind, "long_lists", False)))


def _resolve_pairwise_loss(loss):
    """_resolve_loss for the entry points that have kernels for the seven pairwise kinds only."""
    kind, sigma = _resolve_loss(loss)
    if isinstance(kind, _ListwiseKind):
        raise TypeError("this entry point takes the pairwise losses only (the listwise ones: FusedLinearLoss, "
                        "linear_loss_step, LinearScorer; on the MLP scorer: FusedMLPListwiseLoss, mlp_loss_step)")
    return kind, sigma


def _padded_rows(xs):
    """A (B, L, F) view whose rows sit a multiple of four floats apart -- F4 = (F + 3) & ~3 > F, what
    ``RaggedQueries(pad_features_to=4)`` collates (feature counts like Example3's 5, LETOR's 45 / 46: rows that are not
    whole float4 otherwise run the scalar kernels) -- as the (B, L, F4) tensor it lives in, or None.  The hidden
    columns meet zero weights, so any FINITE content is harmless (the collate writes zeros)."""
    # (a bf16 batch -- RaggedQueries(feature_dtype=torch.bfloat16, pad_features_to=8): rows a multiple of EIGHT values
    # apart, whole 16-byte pieces again; F4 below is then that width)
    if xs.dim() != 3 or xs.dtype not in (torch.float32, torch.bfloat16) or not xs.is_cuda:
        return None
    align = 8 if xs.dtype is torch.bfloat16 else 4
    # only batches the collate of this package made: there the hidden columns are zeros.  A user's own view with the same
    # strides (big[..., :5] of an 8-column tensor) may hide NaN / Inf / metadata columns, which nn.Linear ignores and a
    # zero weight does not (NaN * 0): those are copied to a contiguous batch like any other view
    if not getattr(xs, "_ltr_zero_padded_rows", False):
        return None
    B, L, F = xs.shape
    F4 = (F + align - 1) // align * align
    if F4 == F or B == 0 or L == 0 or xs.stride(2) != 1 or xs.stride(1) != F4 or (B > 1 and xs.stride(0) != L * F4):
        return None
    off = xs.storage_offset()
    if off % align != 0 or xs.untyped_storage().nbytes() < xs.element_size() * (off + B * L * F4):
        return None
    return xs.as_strided((B, L, F4), (L * F4, F4, 1), off)


def _bf16_batch(xs):
    """True for a batch the bf16 Linear kernels (include/ltr_linear_bf16.h) take as it is stored: a torch.bfloat16
    (B, L, F) device tensor that needs no gradient itself, outside autocast."""
    return (torch.is_tensor(xs) and xs.dtype is torch.bfloat16 and xs.dim() == 3 and xs.is_cuda
            and not xs.requires_grad and not torch.is_autocast_enabled())


def _prepare_features(xs, bf16=False):
    """The feature batch as the kernels take it: contiguous fp32 (B, L, F') on the device -- F' = F, or the padded
    row width of a `_padded_rows` view (the callers zero-pad the weights to match and crop the gradient).
    `bf16`: the caller has the bf16 kernels (`_LINEAR_BF16`) -- a `_bf16_batch` stays bf16, contiguous with F' % 8 == 0:
    the batch itself where F % 8 == 0 and it is contiguous, the (B, L, F8) tensor a marked `_padded_rows` view lives in,
    else ONE copy that appends zero columns up to a multiple of 8 (as `_zero_pad` does for the MLP); no fp32 copy is ever
    made.  Every other dtype, and every caller without them (the listwise steps, the lazy launch, the MLP's fp32
    families), casts."""
    if xs.dtype is torch.float32 and xs.is_cuda and xs.dim() == 3 and xs.is_contiguous():
        return xs                                   # the common case: nothing to do
    if bf16 and _bf16_batch(xs):
        extra = (-xs.shape[2]) % 8
        if extra == 0:
            if xs.is_contiguous() and xs.data_ptr() % 16 != 0:      # (a contiguous view at an odd offset: rows off 16 bytes)
                return xs.clone()
            return xs if xs.is_contiguous() else xs.contiguous()
        padded = _padded_rows(xs)
        return padded if padded is not None else torch.nn.functional.pad(xs, (0, extra))
    _C.require_device(xs, "xs")
    if xs.dim() != 3:
        raise ValueError("features must have shape (batch, list_size, features)")
    if xs.dtype != torch.float32:
        xs = xs.float()
    padded = _padded_rows(xs)
    return padded if padded is not None else xs.contiguous()


def _pad_weight(W, Fp):
    """W (F elements) zero-padded to the feature tensor's row width Fp."""
    if W.numel() == Fp:
        return W
    out = torch.zeros(Fp, dtype=torch.float32, device=W.device)
    out[:W.numel()] = W
    return out


def _flat_f32(t, count):
    """A parameter as a contiguous fp32 vector of `count` elements (no copy in the common case)."""
    if t.dtype is torch.float32 and t.is_contiguous() and t.numel() == count:
        return t
    return t.detach().reshape(count).float().contiguous()


class _ShapeOnly:
    def __init__(self, *shape):
        self.shape = torch.Size(shape)


def _labels_and_n(relevance, n, B, L, dev):
    """relevance / n as the C ABI takes them; the generic normalisation only when needed."""
    if (relevance.dtype in _LABEL_CODE and relevance.is_contiguous() and relevance.device == dev
            and relevance.dim() in (2, 3) and relevance.shape[0] == B and relevance.shape[1] == L
            and relevance.numel() == B * L):
        r = relevance
    else:
        r = prepare_relevance(relevance, _ShapeOnly(B, L))
        if r.device != dev:
            raise RuntimeError("features and relevance must be on the same device")
    if (n.dtype is torch.int64 and n.dim() == 1 and n.shape[0] == B and n.is_contiguous()
            and n.device == dev):
        nn = n
    else:
        nn = prepare_n(n, B)
        if nn.device != dev:
            raise RuntimeError("features and n must be on the same device")
    return r, nn


_LABEL_CODE = {torch.int64: _C.LABEL_I64, torch.float32: _C.LABEL_F32, torch.int32: _C.LABEL_I32}
_linear_ws_cache = {}       # (B, L, F) -> ltr_linear_workspace_bytes


def _linear_ws_bytes(B, L, F):
    key = (B, L, F)
    v = _linear_ws_cache.get(key)
    if v is None:
        v = _linear_ws_cache[key] = max(int(_C.lib().ltr_linear_workspace_bytes(B, L, F)), 4)
    return v


class _LinearFamily(collections.namedtuple("_LinearFamily", "name dtype align scores grad grad_ws partials")):
    """The Linear scorer's kernels for one element type of the batch (the twin of `_MLPFamily`): the type, the number of
    values its rows are a multiple of in memory, and the names of its entry points -- scores, weight gradient and its
    workspace size, and the fused step's per-query rows."""
    __slots__ = ()


_LINEAR_F32 = _LinearFamily("f32", torch.float32, 4, "ltr_linear_scores_f32", "ltr_linear_grad_f32",       # include/ltr_hip.h
                            "ltr_linear_grad_workspace_bytes", "ltr_linear_partials_f32")
_LINEAR_BF16 = _LinearFamily("bf16", torch.bfloat16, 8, "ltr_linear_scores_bf16", "ltr_linear_grad_bf16",  # include/ltr_linear_bf16.h
                             "ltr_linear_grad_workspace_bytes_bf16", "ltr_linear_partials_bf16")


def _linear_family_of(X):
    """The family of a prepared batch."""
    return _LINEAR_BF16 if X.dtype is torch.bfloat16 else _LINEAR_F32


def _linear_prepare(xs, weight, relevance, n, kind, raw=None):
    """Check and prepare the batch of a fused launch: ``(X, r, nn, (B, L, F), Fw)`` -- the batch as the kernels take it
    (`_prepare_features`; bf16 stays bf16 for the pairwise kinds, the listwise step is fp32-only), labels and list
    lengths as the C ABI takes them, F the row width in memory and Fw <= F the logical feature count.  The parameters are
    not touched (`_linear_launch` flattens them): a lazily updated one answers every question through a Python hook.

    The weight count is checked against the feature count of `xs`.  A listwise kind is handed the batch as the route
    prepared it (the plan is asked about the rows in memory), so there the weight states the logical count and has to
    fit the rows.  `raw`: the batch as linear_loss_step got it -- its feature count is taken unchecked (a weight of
    another length fails where it is flattened)."""
    listwise = isinstance(kind, _ListwiseKind)
    X = _prepare_features(xs, bf16=not listwise)
    B, L, F = X.shape                           # (F: the row width in memory, >= the logical feature count)
    if raw is not None:
        Fw = raw.shape[2]
    else:
        Fw = weight.numel()
        if listwise:
            if not F - 4 < Fw <= F:
                raise ValueError("weight has %d elements, the feature rows %d" % (Fw, F))
        elif Fw != xs.shape[2]:
            raise ValueError("weight has %d elements, features have %d" % (Fw, xs.shape[2]))
    r, nn = _labels_and_n(relevance, n, B, L, X.device)
    return X, r, nn, (B, L, F), Fw


def _linear_launch(kind, sigma, X, weight, bias, r, nn, dims, Fw, want_scores=False, empty=False):
    """The fused launch on a prepared batch: ``(loss[B], rows, scores | None)`` -- the family's partials entry point
    (ltr_linear_partials_f32 / _bf16) for a pairwise kind, ltr_linear_listwise_partials_f32 for a listwise one (ListMLE
    draws its tie seed here, one per launch), ltr_linear_lambdarank_partials_f32 for LambdaRank.  `rows`: the workspace,
    the (B, PF) per-query gradient rows first, which `_reduce_rows` / ltr_linear_reduce_loss_f32 sum.  An empty batch
    launches nothing unless `empty` (linear_loss_step hands it to the entry point)."""
    B, L, F = dims
    W = _pad_weight(_flat_f32(weight, Fw), F)
    bvec = None if bias is None else _flat_f32(bias, 1)
    dev = X.device
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    ws = torch.empty(_linear_ws_bytes(B, L, F) // 4, dtype=torch.float32, device=dev)
    scores = torch.empty((B, L), dtype=torch.float32, device=dev) if want_scores else None
    if B > 0 or empty:
        listwise = isinstance(kind, _ListwiseKind)
        if listwise:
            from . import _ties
            sd = _ties.draw_seed(L, dev) if kind.loss == _C.LISTWISE_LISTMLE else None
        with _C.device_ctx(X):
            lib = _C.lib()
            bp = None if bvec is None else bvec.data_ptr()
            sp = None if scores is None else scores.data_ptr()
            if listwise and kind.loss == _C.LISTWISE_LAMBDARANK:
                rc = lib.ltr_linear_lambdarank_partials_f32(
                    int(kind.k or 0), float(sigma), X.data_ptr(), W.data_ptr(), bp, r.data_ptr(), _LABEL_CODE[r.dtype],
                    nn.data_ptr(), B, L, F, loss.data_ptr(), sp, ws.data_ptr(), _C.stream_of(X))
            elif listwise:
                rc = lib.ltr_linear_listwise_partials_f32(
                    kind.loss, int(kind.k or 0), X.data_ptr(), W.data_ptr(), bp, r.data_ptr(), _LABEL_CODE[r.dtype],
                    nn.data_ptr(), *_ties.tie_args(sd), B, L, F, loss.data_ptr(), sp, ws.data_ptr(), _C.stream_of(X))
            else:
                rc = getattr(lib, _linear_family_of(X).partials)(
                    kind, float(sigma), X.data_ptr(), W.data_ptr(), bp, r.data_ptr(), _LABEL_CODE[r.dtype],
                    nn.data_ptr(), B, L, F, loss.data_ptr(), sp, ws.data_ptr(), _C.stream_of(X))
            if rc != 0:
                _C.check(rc)
    return loss, ws, scores


class _LinearLossFunction(torch.autograd.Function):
    """loss[b] of `kind` -- a pairwise kind, or a `_ListwiseKind` on a batch `_linear_routed` prepared -- on
    Linear(F, 1)(xs) as ONE launch; backward is the cross-query reduction of its rows (`_reduce_rows`)."""

    @staticmethod
    def forward(ctx, xs, weight, bias, relevance, n, kind, sigma, want_scores):
        X, r, nn, dims, Fw = _linear_prepare(xs, weight, relevance, n, kind)
        B, L, F = dims
        ctx.dims = (B, F)
        ctx.Fw = Fw
        ctx.w_shape = weight.shape
        ctx.has_bias = bias is not None
        # parameters that pytorchltr_amd.optim.SGD updates lazily: the lazy launch (this batch's rows + the previous
        # step's update in ONE launch); its backward and the optimizer step then launch nothing
        st = getattr(weight, "_ltr_lazy", None)
        if st is not None:
            # (there is no bf16 and no listwise lazy launch: such a step settles the pending update and takes the ordinary path)
            if (X.dtype is torch.float32 and not want_scores and bias is not None and Fw == F and ctx.needs_input_grad[1]
                    and ctx.needs_input_grad[2] and getattr(bias, "_ltr_lazy", None) is st
                    and not isinstance(kind, _ListwiseKind)):
                loss = st.forward(ctx, X, r, _LABEL_CODE[r.dtype], nn, kind, sigma)
                if loss is not None:
                    ctx.lazy_loss = loss.detach()            # (an alias without the autograd node: no reference cycle)
                    ctx.save_for_backward(X, r, nn)
                    ctx.lazy_args = (kind, sigma)
                    return loss
            st.settle()                                      # the ordinary path reads the weights: no update may be pending
        loss, ws, scores = _linear_launch(kind, sigma, X, weight, bias, r, nn, dims, Fw, want_scores)
        ctx.save_for_backward(ws)
        if want_scores:
            ctx.mark_non_differentiable(scores)
            return loss, scores
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, *unused):
        lz = getattr(ctx, "lazy", None)
        if lz is not None:
            st = lz[0]
            out = st.backward(ctx, grad_loss)
            if out is not None:
                return (None, out[0], out[1], None, None, None, None, None)
            # an upstream gradient that is not one broadcast scalar (per-query weights): the rows again, the ordinary way
            # (the weights have not moved since the forward pass: no step can have been taken on this gradient)
            if lz[1] != st.gen:
                raise RuntimeError("the gradient rows of this forward pass are gone (a second backward pass through a "
                                   "lazily updated scorer after later training steps)")
            X, r, nn = ctx.saved_tensors
            B, L, F = X.shape
            kind, sigma = ctx.lazy_args
            _, ws, _ = _linear_launch(kind, sigma, X, st.w_raw, st.b_raw, r, nn, (B, L, F), F)
        else:
            (ws,) = ctx.saved_tensors
        dW, db = _reduce_rows(ctx, ws, grad_loss)
        return (None, dW, db, None, None, None, None, None)


def _reduce_rows(ctx, ws, grad_loss):
    """The backward pass of a fused Linear step: (weight.grad, bias.grad) = the per-query rows `ws` of the forward pass
    summed with the upstream gradient as weights (ctx: dims, Fw, w_shape, has_bias)."""
    B, F = ctx.dims
    go = grad_loss
    dW = torch.empty(F, dtype=torch.float32, device=ws.device)
    db = torch.empty(1, dtype=torch.float32, device=ws.device)
    # `.mean().backward()` / `.sum().backward()`: autograd hands over an expanded scalar (stride 0) -- the reduction
    # reads it where it is instead of a (B,) copy being made first
    if B == 0:                                  # (an empty batch: its upstream gradient has no storage to point the reduction at)
        return dW.zero_()[:ctx.Fw].reshape(ctx.w_shape), (db.zero_() if ctx.has_bias else None)
    bcast = go.dtype is torch.float32 and go.dim() == 1 and go.stride(0) == 0
    if not bcast and (go.dtype is not torch.float32 or go.dim() != 1 or not go.is_contiguous()):
        go = go.reshape(B).float().contiguous()
    with _C.device_ctx(ws):
        entry = _C.lib().ltr_linear_reduce_bcast_f32 if bcast else _C.lib().ltr_linear_reduce_f32
        rc = entry(ws.data_ptr(), go.data_ptr(), B, F, dW.data_ptr(), db.data_ptr(), _C.stream_of(ws))
        if rc != 0:
            _C.check(rc)
    return dW[:ctx.Fw].reshape(ctx.w_shape), (db if ctx.has_bias else None)


def _listwise_pieces(scores, relevance, n, kind, sigma=1.0):
    """The stand-alone listwise loss on computed scores (autograd-connected to them); `sigma`: LambdaRank's."""
    from .loss import listwise as _lw
    if kind.loss == _C.LISTWISE_LAMBDARANK:
        from .loss import pairwise_lambda as _pl
        return _pl._LambdaRankFunction.apply(scores, relevance, n, kind.k, sigma)
    if kind.loss == _C.LISTWISE_LISTMLE:
        return _lw._ListMLEFunction.apply(scores, relevance, n, kind.k)
    return _lw._ListwiseSoftmaxFunction.apply(scores, relevance, n)


def _loss_pieces(scores, relevance, n, kind, sigma):
    """The stand-alone loss of `kind`, pairwise or listwise, on computed scores."""
    if isinstance(kind, _ListwiseKind):
        return _listwise_pieces(scores, relevance, n, kind, sigma)
    return _pairwise_pieces(scores, relevance, n, kind, sigma)


# ---- the route table: which kernels a batch reaches from each caller ----
_LIN_F32, _LIN_BF16_FUSED, _LIN_LISTWISE = "f32 fused", "bf16 fused", "listwise fused"
_LIN_F32_PIECES, _LIN_BF16_PIECES, _LIN_SCORES = "f32 pieces", "bf16 pieces", "scores"
_LIN_PIECES = (_LIN_F32_PIECES, _LIN_BF16_PIECES)
_listwise_plan_cache = {}
_pieces_cache = {}
_bf16_plan_cache = {}


def _listwise_fused(kind, X):
    """True where the one-launch listwise step takes the prepared feature batch X (ltr_linear_listwise_plan: lists of
    at most max_list_len() documents, rows of whole float4 that fit the LDS next to the ranked row, at a 16-byte
    aligned address; LambdaRank: ltr_linear_lambdarank_plan, the same rule), else the three kernels -- scorer, listwise
    loss, weight gradient -- compute the same.  (The plan depends on the device: its launch shapes follow the CU count.)"""
    B, L, F = X.shape
    key = (kind.loss, X.device.index, B, L, F)
    v = _listwise_plan_cache.get(key)
    if v is None:
        if len(_listwise_plan_cache) > 1024:
            _listwise_plan_cache.clear()
        with _C.device_ctx(X):
            if kind.loss == _C.LISTWISE_LAMBDARANK:
                v = bool(_C.lib().ltr_linear_lambdarank_plan(B, L, F))
            else:
                v = bool(_C.lib().ltr_linear_listwise_plan(kind.loss, B, L, F))
            _listwise_plan_cache[key] = v
    return v and X.data_ptr() % 16 == 0


def _linear_bf16_plan(kind, B, L, F8):
    """True where ltr_linear_partials_bf16 takes the shape (ltr_linear_bf16_plan; F8: the row width in memory)."""
    key = (int(kind), B, L, F8)
    v = _bf16_plan_cache.get(key)
    if v is None:
        v = _bf16_plan_cache[key] = _C.lib().ltr_linear_bf16_plan(int(kind), B, L, F8) == _C.PLAN_REGISTER_TILE
    return v


def _prefer_pieces(kind, B, L, F, cus=None, plan=None, exempt=True):
    """True where the three-kernel pieces (streaming scorer, split-query loss, streaming weight gradient) beat the
    one-kernel fused step: a few long lists -- one workgroup per query cannot fill the GPU -- whose stand-alone loss has a
    split-query form.  `exempt`: not where the cluster or the parts kernel takes the shape (`plan`: the answer of
    ltr_linear_fused_plan, asked when None); they are fp32 kernels, a bf16 batch passes False.  `cus`: the device's CU
    count, read from the current device when None.  The library's own answers are cached per shape.

    Measured on MI355X, fused kernel -> pieces, us (B x L x F; hinge / logistic / LambdaNDCG2):
      32 x 1000 x 220:  78/136/173 -> 46/52/77      128 x 1000 x 220: 84/145/181 -> 55/66/93
      256 x 1000 x 220: 86/145/183 -> 87/113/147    384 x 1000 x 220: 90/149/186 -> 114/149/204
      128 x 600 x 136:  41/64/90 -> 39/47/72        256 x 600 x 136:  44/66/93 -> 48/60/89
    The cluster kernel (features once, a query over several workgroups) beats the pieces wherever it applies:
    32 x 1000 x 220 hinge 32 vs 46 us, logistic 43 vs 52 -- and so does the parts kernel (round 4, module forward +
    backward replayed, pieces vs fused: 64 x 512 x 700 LambdaNDCG2 91 vs 48 us, 100 x 1000 x 700 hinge 120 vs 78)."""
    cached = exempt and cus is None and plan is None
    if cached:
        v = _pieces_cache.get((kind, B, L, F))
        if v is not None:
            return v
    v = False
    if B > 0 and _C.lib().ltr_pairwise_loss_workspace_bytes(int(kind), B, L) != 0:
        if cus is None:
            cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
        heavy_pairs = kind not in (_C.HINGE, _C.DCG_HINGE)
        v = (2 * B <= cus) or (heavy_pairs and B <= cus and L > 768)
        if v and exempt:
            if plan is None:
                plan = _C.lib().ltr_linear_fused_plan(int(kind), B, L, F)
            v = plan not in (_C.PLAN_CLUSTER, _C.PLAN_PARTS)
    if cached:
        _pieces_cache[(kind, B, L, F)] = v
    return v


def _linear_route(caller, dtype, dim, is_cuda, requires_grad, autocast, kind, B, L, F, cus=None, Fq=None,
                  computed=False, fused_plan=None, listwise_plan=False):
    """Which kernels run ``loss_fn(Linear(F, 1)(xs), ...)`` for a batch of these plain values: _LIN_F32 / _LIN_BF16_FUSED
    (ltr_linear_partials_f32 / _bf16 and the reduction), _LIN_LISTWISE (ltr_linear_listwise_partials_f32 and the
    reduction), _LIN_F32_PIECES / _LIN_BF16_PIECES (the scorer, the stand-alone loss on the fp32 scores, the
    weight-gradient kernel: the fp32 pair, which casts anything that is not fp32, or the bf16 pair) or _LIN_SCORES (the
    scores are computed, or have been: LazyScores.fused_loss answers None, as it does for the pieces).

    `caller`: "step" (linear_loss_step: fused wherever a fused kernel takes the shape), "module" (FusedLinearLoss) or
    "lazy" (a loss module on LazyScores; `computed`: the scores exist already) -- the last two also take the pieces where
    `_prefer_pieces` prefers them.  `kind`: a pairwise kind (a LongKind with its flag) or a `_ListwiseKind`.  `F`: the
    logical feature count (the bf16 rows are zero-padded to a multiple of 8); `Fq`: the count the fp32 pieces rule is
    asked with where the caller has another one (FusedLinearLoss: in_features; LazyScores: F rounded up to 4 for a batch
    that is not contiguous).  What only the library on a device answers comes in as plain values: `cus` and
    `fused_plan` (`_prefer_pieces` asks where None) and `listwise_plan` (the caller's `_listwise_fused`: the listwise
    plan takes the rows as they lie in memory, 16-byte aligned).  A batch that is no (B, L, F) device tensor takes the
    fused fp32 route, whose prepare step raises."""
    if computed:
        return _LIN_SCORES
    bf16 = dtype is torch.bfloat16 and dim == 3 and is_cuda and not requires_grad and not autocast   # (`_bf16_batch`)
    pieces = _LIN_BF16_PIECES if bf16 else _LIN_F32_PIECES
    if isinstance(kind, _ListwiseKind):                  # (no bf16 fused step: a bf16 batch on the plan is cast)
        return _LIN_LISTWISE if listwise_plan else pieces
    if kind == _LISTWISE_SOFTMAX:                        # (the stand-alone softmax kernel as a plain kind: real scores)
        return _LIN_SCORES
    if dim != 3 or not is_cuda:
        return _LIN_F32
    if _long_pair_shape(kind, L):
        return pieces                                    # past max_list_len() (long_lists=True) they are the only path
    if bf16:
        if not _linear_bf16_plan(kind, max(B, 1), L, (F + 7) & ~7):
            return pieces
        if caller != "step" and _prefer_pieces(kind, B, L, F, cus, exempt=False):
            return pieces
        return _LIN_BF16_FUSED
    if caller != "step" and _prefer_pieces(kind, B, L, F if Fq is None else Fq, cus, fused_plan):
        return pieces
    return _LIN_F32


def _linear_routed(caller, xs, kind, Fq=None, computed=False):
    """``(route, batch)``: `_linear_route` on a batch -- its dtype, shape and flags, the autocast state, the library's
    answers -- and the batch to hand on: `xs`, or for a listwise kind the prepared fp32 batch the plan was asked about."""
    if computed:
        return _LIN_SCORES, xs
    X, plan = xs, False
    if isinstance(kind, _ListwiseKind):
        X = _prepare_features(xs)
        plan = _listwise_fused(kind, X)
    elif not torch.is_tensor(xs) or xs.dim() != 3:
        return _LIN_F32, xs
    B, L, F = X.shape
    if caller == "lazy" and not xs.is_contiguous():
        Fq = (F + 3) & ~3
    return _linear_route(caller, xs.dtype, 3, xs.is_cuda, xs.requires_grad, torch.is_autocast_enabled(), kind, B, L, F,
                         None, Fq, False, None, plan), X


def _linear_route_of(caller, xs, kind):
    """The route of `_linear_routed` alone."""
    return _linear_routed(caller, xs, kind)[0]


def _init_linear_parameters(weight, bias, in_features):
    """The initialisation of ``torch.nn.Linear(in_features, 1)``."""
    torch.nn.init.kaiming_uniform_(weight, a=math.sqrt(5))
    if bias is not None:
        bound = 1.0 / math.sqrt(in_features)
        torch.nn.init.uniform_(bias, -bound, bound)


class FusedLinearLoss(torch.nn.Module):
    """``loss_fn(Linear(in_features, 1)(xs), relevance, n)`` as one fused op.

    Gradients flow to ``weight`` and ``bias`` (not to ``xs``: features are data).
    """

    def __init__(self, in_features, loss="hinge", bias=True):
        super().__init__()
        self.in_features = in_features
        self.kind, self.sigma = _resolve_loss(loss)
        self.weight = torch.nn.Parameter(torch.empty(1, in_features))
        self.bias = torch.nn.Parameter(torch.empty(1)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        _init_linear_parameters(self.weight, self.bias, self.in_features)

    def forward(self, xs, relevance, n, return_scores=False):
        if isinstance(self.kind, _ListwiseKind) and self.weight.numel() != xs.shape[-1]:
            raise ValueError("weight has %d elements, features have %d" % (self.weight.numel(), xs.shape[-1]))
        route, X = _linear_routed("module", xs, self.kind, self.in_features)
        if route in _LIN_PIECES:
            # a few long lists (the balanced pieces are faster), a shape no fused kernel takes (there they are the only path)
            scores = _LinearScoreFunction.apply(xs, self.weight, self.bias, n)
            loss = _loss_pieces(scores, relevance, n, self.kind, self.sigma)
            return (loss, scores.detach().squeeze(-1)) if return_scores else loss
        return _LinearLossFunction.apply(X, self.weight, self.bias, relevance, n, self.kind, self.sigma,
                                         bool(return_scores))

    def _prefer_pieces(self, B, L):
        return _prefer_pieces(self.kind, B, L, self.in_features)


def linear_loss_step(xs, weight, bias, relevance, n, loss="hinge", grad_out=None,
                     return_scores=False, return_loss_sum=False):
    """One fused fwd+bwd step without autograd: returns (loss[B], dW[F], db[1][, scores][, loss_sum]).

    dW/db are the gradients of ``sum_b grad_out[b] * loss[b]``; grad_out=None means the
    ``.mean()`` of the reference's training loop (1/B each).  Two launches: the fused
    scorer+loss kernel and the cross-query reduction (which also totals the loss)."""
    kind, sigma = _resolve_loss(loss)
    route, X = _linear_routed("step", xs, kind)
    if route in _LIN_PIECES:
        return _step_pieces(xs, weight, bias, relevance, n, kind, sigma, grad_out, return_scores, return_loss_sum)
    X, r, nn, dims, Fw = _linear_prepare(X, weight, relevance, n, kind, raw=xs)
    B, L, F = dims                                  # (F: the row width in memory -- a padded view's F4)
    lossv, ws, scores = _linear_launch(kind, sigma, X, weight, bias, r, nn, dims, Fw, return_scores, empty=True)
    dW = torch.empty(F, dtype=torch.float32, device=X.device)
    db = torch.empty(1, dtype=torch.float32, device=X.device)
    lsum = torch.zeros(1, dtype=torch.float32, device=X.device) if return_loss_sum else None
    go = None if grad_out is None else grad_out.reshape(B).float().contiguous()
    with _C.device_ctx(X):
        _C.check(_C.lib().ltr_linear_reduce_loss_f32(
            _C.ptr(ws), _C.ptr(go), _C.ptr(lossv), B, F, _C.ptr(dW), _C.ptr(db), _C.ptr(lsum), _C.stream_of(X)))
    out = (lossv, dW[:Fw], db)
    if return_scores:
        out = out + (scores,)
    if return_loss_sum:
        out = out + (lsum,)
    return out


def _step_pieces(xs, weight, bias, relevance, n, kind, sigma, grad_out, return_scores, return_loss_sum):
    """linear_loss_step on a shape no fused launch takes (a listwise loss off its plan; a pairwise loss with
    long_lists=True past max_list_len() documents; a bf16 batch off the plan of its tile): the scorer, the stand-alone
    loss and the weight-gradient kernel, chained by autograd on detached copies of the parameters."""
    B = xs.shape[0]
    with torch.enable_grad():
        w = weight.detach().float().reshape(1, -1).requires_grad_(True)
        b = (torch.zeros(1, dtype=torch.float32, device=xs.device) if bias is None
             else bias.detach().float().reshape(1)).requires_grad_(True)
        scores = _LinearScoreFunction.apply(xs, w, b, n)
        lossv = _loss_pieces(scores, relevance, n, kind, sigma)
        go = (torch.full((B,), 1.0 / max(B, 1), dtype=torch.float32, device=xs.device) if grad_out is None
              else grad_out.reshape(B).float())
        (lossv * go).sum().backward()
    lossv = lossv.detach()
    out = (lossv, w.grad.reshape(-1), b.grad)
    if return_scores:
        out = out + (scores.detach().squeeze(-1),)
    if return_loss_sum:
        out = out + (lossv.sum().reshape(1),)
    return out


class LazySGD:
    """The reference's training loop body, one batch per call as the DataLoader hands them over, with the optimiser
    step applied LAZILY (include/ltr_hip.h: ltr_linear_sgd_lazy_step_f32; examples/01-basic-usage.py:66-75):

        opt = LazySGD(weight, bias, lr, loss="hinge")
        for xs, ys, n in loader:
            opt.step(xs, ys, n)         # loss_fn(Linear(F, 1)(xs), ys, n).mean().backward(); SGD.step()
        opt.flush()                     # the last batch's update; also before the weights are read in between

    `step` launches ONE kernel: it computes this batch's per-query gradient rows and applies the PREVIOUS batch's
    update inside the same launch (its first workgroups sum that batch's rows and hand the new weights to every
    workgroup before the dot products), so the reduction launch and a kernel boundary per step are gone.  Weights,
    gradients and losses are bit-identical to the eager step's.  `weight` (F elements) / `bias` (one element) are
    contiguous fp32 device tensors, updated in place; every batch must have the same (B, L, F).  There is no bf16 lazy
    launch: a ``torch.bfloat16`` batch is cast to fp32 in every ``step`` (train on it through ``linear_loss_step`` or the
    modules instead, which take it as it is stored).

    Data parallel (one process per GPU, every rank steps through its shard of each global batch):
    ``LazySGD(weight, bias, lr, loss, mailbox=MailboxOverlap(F, count=B_shard, device=dev))`` -- the step stays ONE launch
    per rank: the reducer workgroups all-reduce their column sums through the peers' mailboxes inside the launch
    (include/ltr_hip.h: ltr_linear_sgd_lazy_step_dp_f32); all ranks hold bit-identical weights after every step and
    the update is the gradient of the mean over the GLOBAL batch (`mailbox.global_count` queries)."""

    def __init__(self, weight, bias, lr, loss="hinge", mailbox=None):
        self.kind, self.sigma = _resolve_pairwise_loss(loss)
        if weight.dtype is not torch.float32 or not weight.is_contiguous() or not weight.is_cuda:
            raise ValueError("weight must be a contiguous fp32 device tensor (it is updated in place)")
        if bias is None or bias.dtype is not torch.float32 or bias.numel() != 1 or not bias.is_cuda:
            raise ValueError("bias must be an fp32 device tensor of one element (it is updated in place)")
        self.weight, self.bias, self.lr = weight, bias, float(lr)
        if mailbox is not None and not getattr(mailbox, "ok", False):
            raise ValueError("the mailbox is not usable (%s): take RcclOverlap.sgd_step instead" % getattr(mailbox, "why", "?"))
        self.mailbox = mailbox
        self._mb = None if mailbox is None else mailbox.mbox
        self._scale = 0.0 if mailbox is None else 1.0 / float(mailbox.global_count)
        self.pending = 0
        self.shape = None
        self.loss = self.bucket = self.ws = None

    def step(self, xs, relevance, n):
        X = _prepare_features(xs)                   # (no bf16 lazy launch: a bf16 batch is cast to fp32 here, every step)
        B, L, F = X.shape
        if self.shape is None:
            if self.weight.numel() != F:
                raise ValueError("weight has %d elements, the rows %d features" % (self.weight.numel(), F))
            self.shape = (B, L, F)
            dev = X.device
            self.loss = torch.empty(B, dtype=torch.float32, device=dev)
            self.bucket = torch.zeros(F + 2, dtype=torch.float32, device=dev)
            self.ws = torch.empty(_linear_ws_bytes(B, L, F) // 4, dtype=torch.float32, device=dev)
        elif tuple(X.shape) != self.shape:
            raise ValueError("every batch must have the shape of the first one %r (flush() and make a new LazySGD otherwise)" % (self.shape,))
        r, nn = _labels_and_n(relevance, n, B, L, X.device)
        with _C.device_ctx(X):
            _C.check(_C.lib().ltr_linear_sgd_lazy_step_dp_f32(
                self.kind, float(self.sigma), _C.ptr(X), self.weight.data_ptr(), self.bias.data_ptr(), _C.ptr(r),
                _C.label_dtype(r), _C.ptr(nn), B, L, F, self.lr, self.loss.data_ptr(), self.bucket.data_ptr(),
                self.ws.data_ptr(), self.ws.numel() * 4, self.pending, self._scale, None, 0, self._mb, _C.stream_of(X)))
        for t in (X, r, nn):
            t.record_stream(torch.cuda.current_stream(X.device))
        self.pending = B

    def flush(self):
        """Applies the pending update; returns (mean loss, dW | db) of the last batch."""
        if self.pending:
            B, L, F = self.shape
            with _C.device_ctx(self.ws):
                _C.check(_C.lib().ltr_linear_sgd_flush_dp_f32(
                    self.kind, self.weight.data_ptr(), self.bias.data_ptr(), self.pending, L, F, self.lr, self._scale, None, 0,
                    self.loss.data_ptr(), self.bucket.data_ptr(), self.ws.data_ptr(), self._mb, _C.stream_of(self.ws)))
            self.pending = 0
        if self.bucket is None:
            return None
        F = self.shape[2]
        count = float(self.shape[0]) if self.mailbox is None else float(self.mailbox.global_count)
        return self.bucket[F + 1] / count, self.bucket[:F + 1]


# ---------------------------------------------------------------------------------------------
# The Linear(F, 1) scorer on its own (unfused drop-in composition)
# ---------------------------------------------------------------------------------------------
class _LinearScoreFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xs, weight, bias, n):
        X = _prepare_features(xs, bf16=True)        # (a bf16 batch stays bf16: ltr_linear_scores_bf16 / ltr_linear_grad_bf16)
        B, L, F = X.shape                           # (F: the row width in memory -- a padded view's F4)
        Fw = xs.shape[2]
        W = _pad_weight(_flat_f32(weight, Fw), F)
        ctx.Fw = Fw
        bvec = None if bias is None else _flat_f32(bias, 1)
        nn = None if n is None else prepare_n(n, B)
        scores = torch.empty(B, L, dtype=torch.float32, device=X.device)
        if B > 0:
            with _C.device_ctx(X):
                entry = getattr(_C.lib(), _linear_family_of(X).scores)
                _C.check(entry(_C.ptr(X), _C.ptr(W), _C.ptr(bvec), _C.ptr(nn), B, L, F, _C.ptr(scores), _C.stream_of(X)))
        # (the layer's input needs a gradient only when it is not the feature batch itself -- a hidden
        # layer's output: the weight is kept for grad_xs = grad_scores (x) weight in that case)
        ctx.xs_grad = bool(ctx.needs_input_grad[0])
        ctx.save_for_backward(X, nn if nn is not None else torch.empty(0, device=X.device),
                              W if ctx.xs_grad else torch.empty(0, device=X.device))
        ctx.xs_shape = xs.shape
        ctx.has_n = nn is not None
        ctx.w_shape = weight.shape
        ctx.has_bias = bias is not None
        return scores.unsqueeze(-1)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_scores):
        X, nn, Wsaved = ctx.saved_tensors
        B, L, F = X.shape
        g = grad_scores.reshape(B, L).float().contiguous()
        lib = _C.lib()
        out = torch.empty(F + 1, dtype=torch.float32, device=X.device)
        family = _linear_family_of(X)
        ws_bytes = getattr(lib, family.grad_ws)(B, L, F)
        ws = torch.empty(max(ws_bytes, 4) // 4, dtype=torch.float32, device=X.device)
        with _C.device_ctx(X):
            _C.check(getattr(lib, family.grad)(
                _C.ptr(X), _C.ptr(g), _C.ptr(nn) if ctx.has_n else None,
                B, L, F, _C.ptr(out), _C.ptr(ws), ws_bytes, _C.stream_of(X)))
        gx = None
        if ctx.xs_grad:
            gm = g
            if ctx.has_n:                                       # padded documents were not scored
                gm = g * (torch.arange(L, device=g.device)[None, :] < nn[:, None])
            gx = (gm.unsqueeze(-1) * Wsaved.reshape(-1)[:ctx.Fw].reshape(1, 1, ctx.Fw)).reshape(ctx.xs_shape)
        return (gx, out[:ctx.Fw].reshape(ctx.w_shape), out[F:] if ctx.has_bias else None, None)


class LazyScores(torch.Tensor):
    """``Linear(F, 1)(xs)`` that has not been computed yet.

    What :class:`LinearScorer` returns in a training step: a (B, L, 1) fp32 tensor -- shape, dtype and device answer
    without any work -- that remembers ``(xs, weight, bias)``.  The loss modules of this package recognise it and run
    the features-once fused kernel (scores, loss, gradient and the per-query weight-gradient rows in ONE pass over the
    feature tile; ``.backward()`` is then the cross-query reduction straight into ``weight.grad`` / ``bias.grad``): the
    unchanged user script ``loss_fn(model(xs), ys, n).mean().backward()`` (examples/01-basic-usage.py:66-75,
    docs/source/getting-started.rst:86-101) reaches the kernel that ``FusedLinearLoss`` reaches.  Anybody else who
    touches the tensor -- a metric, ``.detach()``, arithmetic, ``print`` -- gets the real scores: they are computed by
    the streaming scorer kernel on first use (autograd-connected to the layer's parameters) and kept."""

    @staticmethod
    def __new__(cls, xs, weight, bias, n):
        r = torch.Tensor._make_wrapper_subclass(cls, (xs.shape[0], xs.shape[1], 1), dtype=torch.float32, device=xs.device)
        r._xs, r._weight, r._bias, r._n = xs, weight, bias, n
        r._real = None
        r._versions = (weight._version, -1 if bias is None else bias._version)
        return r

    def materialize(self):
        """The real (B, L, 1) scores (computed once, autograd-connected to the layer's parameters)."""
        if self._real is None:
            self._check_versions()
            self._real = _LinearScoreFunction.apply(self._xs, self._weight, self._bias, self._n)
        return self._real

    def _check_versions(self):
        if self._versions != (self._weight._version, -1 if self._bias is None else self._bias._version):
            raise RuntimeError("the scorer's parameters were modified in place between model(xs) and the first use of its "
                               "scores; use the scores (or call .materialize()) before the optimizer step")

    def fused_loss(self, relevance, n, kind, sigma):
        """loss[b] of the loss `kind` (a pairwise kind or a _ListwiseKind) on these scores, or None when the scores have
        to be computed anyway."""
        route, X = _linear_routed("lazy", self._xs, kind, computed=self._real is not None)
        if route is _LIN_SCORES or route in _LIN_PIECES:
            return None
        self._check_versions()
        return _LinearLossFunction.apply(X, self._weight, self._bias, relevance, n, kind, sigma, False)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func in _LAZY_METADATA:
            if func == _REQUIRES_GRAD_GET:
                a = args[0]
                return bool(a._weight.requires_grad or (a._bias is not None and a._bias.requires_grad))
            with torch._C.DisableTorchFunctionSubclass():
                return func(*args, **kwargs)

        with torch._C.DisableTorchFunctionSubclass():
            return func(*[_real_scores(a) for a in args], **{k: _real_scores(v) for k, v in kwargs.items()})

    @classmethod
    def __torch_dispatch__(cls, func, types, args=(), kwargs=None):
        # (only reached by calls that bypass the Python API -- every torch function and Tensor method goes through
        # __torch_function__ above, where autograd still sees the real scores)
        return func(*[_real_scores(a) for a in args], **{k: _real_scores(v) for k, v in (kwargs or {}).items()})


def _real_scores(a):
    """`a` with every LazyScores in it (lists and tuples are searched) replaced by its real scores."""
    if isinstance(a, LazyScores):
        return a.materialize()
    if isinstance(a, (list, tuple)):
        return type(a)(_real_scores(v) for v in a)
    return a


_LISTWISE_SOFTMAX = 100                  # (_autograd.LISTWISE_SOFTMAX as a plain kind: the stand-alone kernel on real scores)
_REQUIRES_GRAD_GET = torch.Tensor.requires_grad.__get__
_LAZY_METADATA = {
    torch.Tensor.shape.__get__, torch.Tensor.dtype.__get__, torch.Tensor.device.__get__, torch.Tensor.is_cuda.__get__,
    torch.Tensor.ndim.__get__, torch.Tensor.layout.__get__, torch.Tensor.size, torch.Tensor.dim, torch.Tensor.numel,
    torch.Tensor.nelement, torch.Tensor.ndimension, torch.Tensor.is_floating_point, torch.Tensor.is_complex,
    torch.Tensor.get_device, _REQUIRES_GRAD_GET,
}


class LinearScorer(torch.nn.Module):
    """``torch.nn.Linear(in_features, 1)`` for (B, L, F) feature batches, state_dict-compatible
    with it, computed by HBM-streaming kernels instead of rocBLAS' one-column GEMM:
    ``loss_fn(scorer(xs), ys, n)`` is the reference's user code unchanged.  ``scorer(xs, n)`` also
    skips the padded documents (score 0).  While gradients are enabled the layer returns :class:`LazyScores`: a loss
    module of this package then runs scores + loss + weight gradient as ONE kernel over the features (what
    ``FusedLinearLoss`` does), anything else that touches the scores computes them on the spot.  The feature batch gets
    no gradient (it is data); an input that requires one (the layer sits behind others) gets
    ``grad_scores (x) weight``.

    ONE difference from ``nn.Linear`` follows from the laziness: scores that are first USED after ``optimizer.step()`` --
    ``scores = model(xs); loss_fn(scores, ys, n).mean().backward(); optimizer.step(); ndcg(scores, ys, n)`` -- would have to
    be computed with weights that no longer exist; that first use raises a RuntimeError instead of returning post-step
    scores.  Use the scores before the step (any use computes and keeps them), call ``scores.materialize()``, or build the
    layer with ``lazy=False`` (``use_linear_scorer`` keeps the default) -- then every call computes its scores at once and
    only the fused ``FusedLinearLoss`` / ``linear_loss_step`` entry points take the one-pass kernel."""

    def __init__(self, in_features, bias=True, lazy=True):
        super().__init__()
        self.in_features = in_features
        self.lazy = lazy
        self.weight = torch.nn.Parameter(torch.empty(1, in_features))
        self.bias = torch.nn.Parameter(torch.empty(1)) if bias else None
        _init_linear_parameters(self.weight, self.bias, in_features)
        if self.bias is not None:
            self.weight._ltr_scorer_bias = self.bias          # (pytorchltr_amd.optim.SGD pairs them up by this)

    def __setstate__(self, state):
        # (copy.deepcopy and unpickling -- torch.load of a whole model -- arrive here with new Parameter objects, which carry
        # no attributes: pair them up again, or the copy would never reach the lazy step)
        super().__setstate__(state)
        if self.bias is not None:
            self.weight._ltr_scorer_bias = self.bias

    def forward(self, xs, n=None):
        if not (torch.is_tensor(xs) and xs.dim() == 3 and xs.is_cuda
                and (xs.dtype is torch.float32 or _bf16_batch(xs))
                and xs.shape[-1] == self.in_features and not torch.is_autocast_enabled()):
            # not an fp32 (B, L, F) feature batch on the device, nor a bf16 one that needs no gradient (a value head, a
            # gate, a 2-D input, half precision under autocast ...): the plain layer, with nn.Linear's dtype rules and errors
            return torch.nn.functional.linear(xs, self.weight, self.bias)
        if (self.lazy and torch.is_grad_enabled() and not xs.requires_grad and (xs.is_contiguous() or _padded_rows(xs) is not None)
                and (self.weight.requires_grad or (self.bias is not None and self.bias.requires_grad))):
            return LazyScores(xs, self.weight, self.bias, n)
        return _LinearScoreFunction.apply(xs, self.weight, self.bias, n)


def use_linear_scorer(model, predicate=None):
    """The one-liner for an existing training script: every ``torch.nn.Linear(F, 1)`` inside `model`
    (or `model` itself) is replaced by a :class:`LinearScorer` that SHARES its parameters -- same
    ``state_dict`` keys, same Parameter objects, so optimisers, checkpoints and ``model.parameters()``
    are unaffected -- and `loss_fn(model(xs), ys, n).mean().backward()` stops paying rocBLAS for a
    one-column GEMM (304 us -> 46 us per step at the C2 shape; reference user code:
    examples/01-basic-usage.py:36,66-75).  Returns the model (a new module when `model` itself was the
    Linear layer).  Only applied where the layer's input is the (B, L, F) feature batch, i.e. where the
    user wrote ``Linear(F, 1)`` as the scorer: `predicate(name, module) -> bool` restricts the replacement (default: every
    ``Linear(*, 1)``); a converted layer that is fed anything but a 3-D device tensor falls back to ``F.linear``."""
    def convert(lin):
        sc = LinearScorer(lin.in_features, bias=lin.bias is not None)
        sc.weight = lin.weight                      # the same Parameter objects
        if lin.bias is not None:
            sc.bias = lin.bias
            sc.weight._ltr_scorer_bias = sc.bias
        return sc

    def is_scorer(m):
        return isinstance(m, torch.nn.Linear) and m.out_features == 1

    if is_scorer(model):
        return convert(model) if (predicate is None or predicate("", model)) else model
    for name, child in list(model.named_children()):
        if is_scorer(child):
            if predicate is None or predicate(name, child):
                setattr(model, name, convert(child))
        else:
            use_linear_scorer(child, predicate)
    return model


# ---------------------------------------------------------------------------------------------
# ReLU MLP scorer (the network of the reference's guide) fused with the loss -- SURVEY.md 8 f-2
# ---------------------------------------------------------------------------------------------
MLP_MAX_LIST_LEN = 128           # feature rows wider than 144 floats
MLP_MAX_LIST_LEN_NARROW = 256    # F <= 144
MLP_NARROW_FEATURES = 144
MLP_MAX_FEATURES = 224
MLP_WIDE_MAX_FEATURES = 704      # the K-streamed kernels of include/ltr_mlp_wide.h (Yahoo: 699 -> 700)
MLP_MAX_HIDDEN = (64, 16)


def mlp_max_list_len(F):
    """Longest list the fused MLP kernels take at F features: 256 for F <= 144 (the tile kernel),
    128 for wider rows (ltr_mlp_max_list_len)."""
    return MLP_MAX_LIST_LEN_NARROW if F <= MLP_NARROW_FEATURES else MLP_MAX_LIST_LEN


def mlp_supported(L, F, H1, H2):
    """Shapes the fused MLP kernel takes (see include/ltr_hip.h: ltr_mlp_pairwise_f32)."""
    return (0 < F <= MLP_MAX_FEATURES and F % 4 == 0 and 0 < L <= mlp_max_list_len(F)
            and 0 < H1 <= MLP_MAX_HIDDEN[0] and 0 < H2 <= MLP_MAX_HIDDEN[1])


class _MLPFamily(collections.namedtuple("_MLPFamily", "name dtype align f_min f_max scores grad grad_ws limits")):
    """One family of stand-alone MLP scorer kernels: the element type of its batch, the alignment and the range
    (f_min, f_max] of its feature counts, the names of its three entry points, the limits as its ValueError states them."""
    __slots__ = ()

    def takes(self, F, H1, H2):
        """Networks the family's kernels take, at any list length."""
        return (self.f_min < F <= self.f_max and F % self.align == 0
                and 0 < H1 <= MLP_MAX_HIDDEN[0] and 0 < H2 <= MLP_MAX_HIDDEN[1])


_MLP_ROWS = _MLPFamily("rows", torch.float32, 4, 0, MLP_MAX_FEATURES,                               # include/ltr_mlp_rows.h
                       "ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32", "ltr_mlp_rows_grad_workspace_bytes",
                       "the MLP row kernels take F <= %d with F %% 4 == 0" % MLP_MAX_FEATURES)
_MLP_WIDE = _MLPFamily("wide", torch.float32, 4, MLP_MAX_FEATURES, MLP_WIDE_MAX_FEATURES,           # include/ltr_mlp_wide.h
                       "ltr_mlp_wide_scores_f32", "ltr_mlp_wide_grad_f32", "ltr_mlp_wide_grad_workspace_bytes",
                       "the wide-row MLP kernels take %d < F <= %d with F %% 4 == 0" % (MLP_MAX_FEATURES, MLP_WIDE_MAX_FEATURES))
_MLP_BF16 = _MLPFamily("bf16", torch.bfloat16, 8, 0, MLP_MAX_FEATURES,    # include/ltr_mlp_bf16.h: rows of whole 16-byte pieces
                       "ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad", "ltr_mlp_bf16_grad_workspace_bytes",
                       "the bf16 MLP kernels take F <= %d (after zero-padding to a multiple of 8)" % MLP_MAX_FEATURES)
_mlp_rows_network, _mlp_wide_network, _mlp_bf16_network = _MLP_ROWS.takes, _MLP_WIDE.takes, _MLP_BF16.takes


def _mlp_family_of(dtype, F, wide=False):
    """The family of a prepared batch: bf16 -> bf16, more than 224 features -> wide, otherwise rows.  `wide` is the
    launchers' earlier flag, which tests/test_gpu_mlp_wide.py still passes: the wide family on rows of any width.
    (Plain values, not the batch: the launchers have F at hand, and a second `X.shape` costs more than this call.)"""
    return _MLP_BF16 if dtype is torch.bfloat16 else _MLP_WIDE if wide or F > MLP_MAX_FEATURES else _MLP_ROWS


def _flat_params(params, F):
    # (fp32 contiguous tensors -- nn.Linear parameters -- go to the C ABI as they are)
    W1, b1, W2, b2, W3, b3 = [t if (t.dtype is torch.float32 and t.is_contiguous())
                              else t.detach().float().contiguous() for t in params]
    H1, H2 = W1.shape[0], W2.shape[0]
    if W1.shape != (H1, F) or b1.numel() != H1 or W2.shape != (H2, H1) or b2.numel() != H2 \
            or W3.numel() != H2 or b3.numel() != 1:
        raise ValueError("parameters must be those of Linear(F,H1), Linear(H1,H2), Linear(H2,1)")
    return (W1, b1, W2, b2, W3, b3), H1, H2


def _split_grads(flat, F, H1, H2):
    """The six gradient tensors as views of the flat buffer [dW1 | db1 | dW2 | db2 | dW3 | db3]."""
    w1, b1, w2, b2, w3, b3 = flat.split((H1 * F, H1, H2 * H1, H2, H2, 1))
    return (w1.view(H1, F), b1, w2.view(H2, H1), b2, w3.view(1, H2), b3)


_mlp_sizes = {}          # (B, F, H1, H2) -> (parameter count, workspace bytes)
_mlp_workspaces = {}     # (device index, stream, bytes) -> scratch tensor (consumed in stream order)


def _mlp_sizes_for(B, F, H1, H2):
    key = (B, F, H1, H2)
    v = _mlp_sizes.get(key)
    if v is None:
        lib = _C.lib()
        v = _mlp_sizes[key] = (int(lib.ltr_mlp_param_count(F, H1, H2)),
                               int(lib.ltr_mlp_workspace_bytes(B, F, H1, H2)))
    return v


def _mlp_workspace(dev, stream, ws_bytes):
    """The per-workgroup partial vectors (15 MB at the guide's network) live only between the two
    launches of one call, which run in stream order: one buffer per (device, stream) is reused."""
    if torch.cuda.is_current_stream_capturing():
        # a buffer allocated under capture belongs to the graph's pool: never cache it
        return torch.empty(max(ws_bytes, 4) // 4, dtype=torch.float32, device=dev)
    key = (dev.index, stream, ws_bytes)
    ws = _mlp_workspaces.get(key)
    if ws is None:
        if len(_mlp_workspaces) > 16:
            _mlp_workspaces.clear()
        ws = _mlp_workspaces[key] = torch.empty(max(ws_bytes, 4) // 4, dtype=torch.float32, device=dev)
    return ws


def mlp_listwise_supported(kind, B, L, F, H1, H2):
    """True where the fused MLP kernels take a listwise loss at this shape (ltr_mlp_listwise_plan: the shapes of
    :func:`mlp_supported` whose ranked row fits the LDS next to the network's).  An empty batch counts as taken."""
    if not mlp_supported(L, F, H1, H2):
        return False
    return B == 0 or bool(_C.lib().ltr_mlp_listwise_plan(kind.loss, B, L, F, H1, H2))


def mlp_lambdarank_supported(B, L, F, H1, H2):
    """True where the fused MLP kernels take LambdaRank at this shape (ltr_mlp_lambdarank_plan: the shapes of
    :func:`mlp_listwise_supported`).  An empty batch counts as taken."""
    if not mlp_supported(L, F, H1, H2):
        return False
    return B == 0 or bool(_C.lib().ltr_mlp_lambdarank_plan(B, L, F, H1, H2))


_mlp_rows_ws = {}        # (device index, B, L, F, H1, H2, family) -> *_grad_workspace_bytes (grows with the CU count)


def _zero_pad(xs, w1, align):
    """Feature counts that are not a multiple of `align` (MQ2007: 46, Yahoo: 699; bf16 rows, whole 16-byte pieces of 8
    values: Istella's 220): zero columns are appended to the features and to W1 -- same scores, and the extra dW1
    columns are dropped (`_crop_grads`).  Costs one copy of the batch; pad the stored split once to avoid it."""
    extra = (-xs.shape[-1]) % align
    if extra == 0:
        return xs, w1, 0
    return torch.nn.functional.pad(xs, (0, extra)), torch.nn.functional.pad(w1.detach(), (0, extra)), extra


def _mlp_prepare(xs, params, family=None, pad=True):
    """The arguments of a family's kernels: ``(X, flat_params, H1, H2, extra, family)`` -- the contiguous batch on the
    device, the fp32 parameters, the hidden sizes, the number of zero columns appended (`pad`; W1 is padded to match)
    and the family, chosen from the batch where None is given (`_mlp_family_of`).  ValueError for a network the family
    does not take.  The f32 families go through `_prepare_features` (any dtype is cast, `_padded_rows` views are
    honoured, the device is checked first); the bf16 family takes bf16 batches only and checks the device last."""
    if family is None and torch.is_tensor(xs) and xs.dtype is torch.bfloat16:
        family = _MLP_BF16
    bf16 = family is _MLP_BF16
    if bf16:
        if not torch.is_tensor(xs) or xs.dtype is not torch.bfloat16:
            raise ValueError("the bf16 MLP kernels take torch.bfloat16 features (fp32 features: mlp_scores / mlp_grad)")
        if xs.dim() != 3:
            raise ValueError("features must have shape (batch, list_size, features)")
    params, extra = list(params), 0
    if pad:
        xs, params[0], extra = _zero_pad(xs, params[0], family.align if family else 4)
    X = xs if bf16 else _prepare_features(xs)
    B, L, F = X.shape
    flat_params, H1, H2 = _flat_params(params, F)
    if family is None:
        family = _mlp_family_of(X.dtype, F)
    if not family.takes(F, H1, H2) or L == 0:
        raise ValueError("%s, hidden <= %s and L >= 1; got L=%d F=%d hidden=(%d, %d)"
                         % (family.limits, MLP_MAX_HIDDEN, L, F - extra, H1, H2))
    if bf16:
        _C.require_device(X, "xs")
        X = X.contiguous()
    return X, flat_params, H1, H2, extra, family


def _mlp_grad_buffer(out, P, dev):
    """The flat gradient buffer of P floats: `out` where the caller preallocated one."""
    flat = out if out is not None else torch.empty(P, dtype=torch.float32, device=dev)
    if flat.numel() != P or flat.dtype != torch.float32 or not flat.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor of %d elements" % P)
    return flat


def _crop_grads(parts, extra, shapes=None):
    """The six gradients without the dW1 columns of `extra` zero-padded features, in the parameters' `shapes`."""
    parts = list(parts)
    if extra:
        parts[0] = parts[0][:, :parts[0].shape[1] - extra]
    return tuple(g if shapes is None or g.shape == s else g.reshape(s) for g, s in zip(parts, shapes or parts))


def _mlp_rows_scores(X, flat_params, H1, H2, nn, wide=False, family=None):
    """The family's score entry point (ltr_mlp_rows_scores_f32, ltr_mlp_wide_scores_f32, ltr_mlp_bf16_scores; None: the
    family of `X`, `_mlp_family_of`) on prepared arguments: (B, L) scores, 0 on the padded documents."""
    B, L, F = X.shape
    scores = torch.empty(B, L, dtype=torch.float32, device=X.device)
    if B > 0:
        fn = getattr(_C.lib(), (family or _mlp_family_of(X.dtype, F, wide)).scores)
        with _C.device_ctx(X):
            _C.check(fn(_C.ptr(X), *[_C.ptr(t) for t in flat_params], _C.ptr(nn), B, L, F, H1, H2, _C.ptr(scores),
                        _C.stream_of(X)))
    return scores


def _mlp_grad_call(X, flat_params, H1, H2, grad_scores, n, out, wide=False, family=None):
    """The family's gradient entry point (ltr_mlp_rows_grad_f32, ltr_mlp_wide_grad_f32, ltr_mlp_bf16_grad; None: the
    family of `X`) behind the shape checks of its caller."""
    B, L, F = X.shape
    dev = X.device
    if grad_scores.numel() != B * L or grad_scores.device != dev:
        raise ValueError("grad_scores must hold one value per document of xs, on its device")
    g = grad_scores.detach().reshape(B, L)
    if g.dtype is not torch.float32 or not g.is_contiguous():
        g = g.float().contiguous()
    nn = None if n is None else prepare_n(n, B)
    lib = _C.lib()
    flat = _mlp_grad_buffer(out, _mlp_sizes_for(max(B, 1), F, H1, H2)[0], dev)
    family = family or _mlp_family_of(X.dtype, F, wide)
    key = (dev.index, B, L, F, H1, H2, family.name)
    with _C.device_ctx(X):
        ws_bytes = _mlp_rows_ws.get(key)
        if ws_bytes is None:                # (asked with X's device current: the grid follows its CU count)
            ws_bytes = _mlp_rows_ws[key] = int(getattr(lib, family.grad_ws)(B, L, F, H1, H2))
        st = _C.stream_of(X)
        ws = _mlp_workspace(dev, st, ws_bytes)
        _C.check(getattr(lib, family.grad)(
            _C.ptr(X), *[_C.ptr(t) for t in flat_params], _C.ptr(g), _C.ptr(nn), B, L, F, H1, H2, _C.ptr(flat),
            _C.ptr(ws), ws_bytes, st))
    return _split_grads(flat, F, H1, H2)


def _mlp_family_scores(xs, params, n, family):
    X, flat_params, H1, H2, _, family = _mlp_prepare(xs, params, family, pad=family is _MLP_BF16)
    return _mlp_rows_scores(X, flat_params, H1, H2, None if n is None else prepare_n(n, X.shape[0]), family=family)


def _mlp_family_grad(xs, params, grad_scores, n, out, family):
    X, flat_params, H1, H2, extra, family = _mlp_prepare(xs, params, family, pad=family is _MLP_BF16)
    return _crop_grads(_mlp_grad_call(X, flat_params, H1, H2, grad_scores, n, out, family=family), extra)


def mlp_grad(xs, params, grad_scores, n=None, out=None):
    """The parameter gradients of ``sum_{b, j < n[b]} grad_scores[b, j] * mlp(xs)[b, j]`` as one row-streaming MFMA
    kernel plus the fixed-order reduction (ltr_mlp_rows_grad_f32; no autograd, any list length): what
    ``scores.backward(grad_scores)`` leaves in the six ``.grad``s.  The activations are recomputed from ``xs``.

    Args:
        xs: (B, L, F) float32 features on the device, F a multiple of 4 and at most 224.
        params: ``(W1, b1, W2, b2, W3, b3)`` in torch layout, hidden sizes up to (64, 16).
        grad_scores: (B, L) or (B, L, 1); entries of padded documents are not read.
        n: (B,) list lengths, or None: every document is real.
        out: optional preallocated flat gradient buffer of ``ltr_mlp_param_count`` floats.

    Returns:
        ``(dW1, db1, dW2, db2, dW3, db3)``, views of one flat buffer as :func:`mlp_loss_step` returns them.
    """
    return _mlp_family_grad(xs, params, grad_scores, n, out, _MLP_ROWS)


def mlp_wide_scores(xs, params, n=None):
    """:func:`mlp_scores` for feature rows wider than 224 floats, up to 704 (ltr_mlp_wide_scores_f32: the feature
    dimension is streamed in chunks; any list length; no autograd): (B, L) float32 scores for documents < n[b] and 0 for
    the padded ones, whose features are not read; n=None scores every document.  Other networks raise ValueError."""
    return _mlp_family_scores(xs, params, n, _MLP_WIDE)


def mlp_wide_grad(xs, params, grad_scores, n=None, out=None):
    """:func:`mlp_grad` for feature rows wider than 224 floats, up to 704 (ltr_mlp_wide_grad_f32): same arguments, same
    ``(dW1, db1, dW2, db2, dW3, db3)`` views of one flat buffer.  Other networks raise ValueError."""
    return _mlp_family_grad(xs, params, grad_scores, n, out, _MLP_WIDE)


def mlp_scores_bf16(xs, params, n=None):
    """:func:`mlp_scores` on a batch kept as ``torch.bfloat16`` (half the bytes of the fp32 batch; any list length; no
    autograd): (B, L) float32 scores for documents < n[b] and 0 for the padded ones, whose features are not read.  One
    row-streaming kernel whose first layer runs on the bf16 MFMA (ltr_mlp_bf16_scores).  The parameters stay fp32; the
    kernel rounds W1 to bf16 (nearest even) for the first layer -- the scores are those of the network with
    ``W1.bfloat16()``, accumulated in fp32 -- everything behind the first layer is fp32.  Feature counts that are not a
    multiple of 8 are zero-padded with one copy.  Other networks raise ValueError."""
    return _mlp_family_scores(xs, params, n, _MLP_BF16)


def mlp_grad_bf16(xs, params, grad_scores, n=None, out=None):
    """:func:`mlp_grad` on a ``torch.bfloat16`` batch (ltr_mlp_bf16_grad): the fp32 gradients of
    ``sum grad_scores * mlp_scores_bf16(xs, params)``, ``dW1`` being the gradient with respect to the rounded W1 the
    forward uses (a straight-through update of the fp32 master weights).  Same arguments and the same
    ``(dW1, db1, dW2, db2, dW3, db3)`` views of one flat buffer; with a feature count that is not a multiple of 8, `out`
    holds the padded network's parameters and ``dW1`` is the view of its first F columns."""
    return _mlp_family_grad(xs, params, grad_scores, n, out, _MLP_BF16)


class _MLPScoreFunction(torch.autograd.Function):
    """``mlp(xs)`` with parameter gradients: forward is the score kernel of the batch's family (`_mlp_family_of`: the
    row kernels, the wide-row pair past 224 features, the bf16 pair on a bf16 batch), backward its gradient kernel on
    ``grad_scores`` (the activations are recomputed; nothing but the prepared batch -- a copy only where the feature
    count had to be padded -- and the parameters is kept).  The features get no gradient (they are data; callers route
    an input that requires one to the torch layers)."""

    @staticmethod
    def forward(ctx, xs, n, *params):
        X, flat_params, H1, H2, extra, family = _mlp_prepare(xs, [t.detach() for t in params])
        nn = None if n is None else prepare_n(n, X.shape[0])
        scores = _mlp_rows_scores(X, flat_params, H1, H2, nn, family=family)
        ctx.save_for_backward(X, nn if nn is not None else torch.empty(0, device=X.device), *flat_params)
        ctx.has_n = nn is not None
        ctx.extra, ctx.family = extra, family
        ctx.shapes = [t.shape for t in params]
        return scores.unsqueeze(-1)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_scores):
        X, nn, *flat_params = ctx.saved_tensors
        H1, H2 = flat_params[0].shape[0], flat_params[2].shape[0]
        parts = _mlp_grad_call(X, flat_params, H1, H2, grad_scores, nn if ctx.has_n else None, None, family=ctx.family)
        return (None, None) + _crop_grads(parts, ctx.extra, ctx.shapes)


# ---- the route table: which kernels a batch reaches from each caller ----
_FUSED, _PER_QUERY, _ROWS, _WIDE, _BF16, _TORCH = "fused step", "per-query scores", "rows", "wide", "bf16", "torch layers"
_ROUTE_FAMILY = {_FUSED: _MLP_ROWS, _PER_QUERY: _MLP_ROWS, _ROWS: _MLP_ROWS, _WIDE: _MLP_WIDE, _BF16: _MLP_BF16}


def _f4(F):
    """The row width of F features after the modules' zero-padding to whole float4."""
    return (F + 3) & ~3


def _mlp_route(caller, dtype, dim, is_cuda, requires_grad, grad_enabled, autocast, L, F, H1, H2, kind=None, plan=True):
    """Which kernels compute ``mlp(xs)`` (and, for a caller with a loss `kind`, the step): plain values in, one of
    _FUSED (the one-launch step, ltr_mlp_pairwise_f32 / ltr_mlp_listwise_f32 / ltr_mlp_lambdarank_f32), _PER_QUERY (ltr_mlp_scores_f32), _ROWS,
    _WIDE, _BF16 (the three families) or _TORCH out -- the three ``nn.Linear`` layers in a module, ValueError in a
    function, which has none.  A family's ValueError (bf16: a network it does not take) is raised by `_mlp_prepare`.

    `caller`: "scorer" (MLPScorer.forward), "score" (the loss modules' score()), "loss" (their forward()), "step"
    (mlp_loss_step), "scores" (mlp_scores).  `plan`: False where a listwise `kind` is off the plan of the fused
    step (:func:`mlp_listwise_supported`, asked by the caller: this function calls nothing).
    The modules zero-pad the feature count to a multiple of 4 (bf16: 8), the functions take it as it is.
    """
    if dim != 3 or not is_cuda or L <= 0:
        return _TORCH
    module = caller in ("scorer", "score", "loss")
    data = not requires_grad and not autocast           # a batch that needs no gradient itself, outside autocast
    if dtype is torch.bfloat16 and data and (module or (caller == "step" and F % 8 == 0)):
        return _BF16                                     # at every list length: the fused kernels are fp32-only
    if module:
        F = _f4(F)                                       # (everything below computes in fp32)
    if kind is not None and plan and mlp_supported(L, F, H1, H2):
        return _FUSED                                    # any dtype (cast to fp32), also a batch that is no `data`
    rows, wide = _MLP_ROWS.takes(F, H1, H2), _MLP_WIDE.takes(F, H1, H2)
    if not module:                                       # any dtype is cast to fp32; no wide route, no torch layers
        if caller == "scores" and rows and L <= mlp_max_list_len(F):
            return _PER_QUERY
        return _ROWS if rows else _TORCH
    if caller != "scorer" and not grad_enabled:          # evaluation through score(): any dtype on the f32 kernels
        if rows:
            return _PER_QUERY if L <= mlp_max_list_len(F) else _ROWS
        return _WIDE if wide and dtype is torch.float32 and not autocast else _TORCH
    f32_data = dtype is torch.float32 and data
    return _ROWS if rows and f32_data else _WIDE if wide and f32_data else _TORCH


def _mlp_route_of(caller, xs, F, H1, H2, kind=None, plan=True):
    """`_mlp_route` on a batch: its dtype, shape and flags, the grad mode and the autocast state (F None: the batch's)."""
    if not torch.is_tensor(xs) or xs.dim() != 3:
        return _TORCH
    _, L, Fx = xs.shape
    return _mlp_route(caller, xs.dtype, 3, xs.is_cuda, xs.requires_grad, torch.is_grad_enabled(),
                      torch.is_autocast_enabled(), L, Fx if F is None else F, H1, H2, kind, plan)


def _mlp_step_pieces(X, flat_params, H1, H2, relevance, n, kind, sigma, grad_out, return_scores, return_loss_sum, out):
    """mlp_loss_step past the limits of the fused kernels, as `_step_pieces` is for the Linear scorer: the row score
    kernel, the stand-alone loss kernel (its d loss / d score scaled by `grad_out`), the row gradient kernel."""
    B, L, F = X.shape
    dev = X.device
    r, nn = _labels_and_n(relevance, n, B, L, dev)
    scores = _mlp_rows_scores(X, flat_params, H1, H2, nn)       # (a bf16 X: the bf16 kernels, here and below)
    with torch.enable_grad():
        s = scores.unsqueeze(-1).requires_grad_(True)
        lossv = (_listwise_pieces(s, r, nn, kind, sigma) if isinstance(kind, _ListwiseKind)
                 else _pairwise_pieces(s, r, nn, kind, sigma))
        go = (torch.full((B,), 1.0 / max(B, 1), dtype=torch.float32, device=dev) if grad_out is None
              else grad_out.reshape(B).float())
        (ds,) = torch.autograd.grad((lossv * go).sum(), s)
    lossv = lossv.detach()
    res = (lossv, _mlp_grad_call(X, flat_params, H1, H2, ds, nn, out))
    if return_scores:
        res = res + (scores,)
    if return_loss_sum:
        res = res + (lossv.sum().reshape(1),)
    return res


def mlp_loss_step(xs, params, relevance, n, loss="hinge", grad_out=None, return_scores=False,
                  return_loss_sum=False, out=None):
    """One fused forward+backward step of ``loss_fn(mlp(xs), relevance, n)`` without autograd.

    Args:
        xs: (B, L, F) float32 features on the device; a ``torch.bfloat16`` batch with F % 8 == 0 runs, at every list
            length, as the three pieces below on the bf16 kernels (:func:`mlp_scores_bf16`, :func:`mlp_grad_bf16`).
        loss: a pairwise kind name or module, or a listwise loss -- ``"listnet"`` / ``"softmax"``, ``"listmle"``,
            ``ListwiseSoftmaxLoss()``, ``ListMLELoss(k)`` (ltr_mlp_listwise_f32; ListMLE draws one tie seed per call,
            as ``ListMLELoss`` does, and ``utils.tie_breaking("index")`` turns it off).
        params: ``(W1, b1, W2, b2, W3, b3)`` of ``Linear(F,H1) / ReLU / Linear(H1,H2) / ReLU /
            Linear(H2,1)`` in torch layout.
        grad_out: (B,) weights of the per-query losses; None = 1/B (the ``.mean()`` of the guide's
            training loop, docs/source/getting-started.rst:95).
        out: optional preallocated flat gradient buffer of ``ltr_mlp_param_count`` floats.

    Lists longer than the fused kernels hold (:func:`mlp_max_list_len`; a listwise loss off its plan) run as three
    pieces instead of one launch -- the row score kernel, the stand-alone loss kernel, the row gradient kernel
    (:func:`mlp_grad`) -- with the same results; a pairwise module needs ``long_lists=True`` past ``max_list_len()``.

    Returns:
        ``(loss[B], grads)`` with ``grads = (dW1, db1, dW2, db2, dW3, db3)`` views of one flat
        buffer (available as ``grads[0].base`` / the ``out`` argument), then optionally the scores
        (valid for documents < n only) and ``loss_sum`` (1,).
    """
    kind, sigma = _resolve_loss(loss)
    if isinstance(kind, _ListwiseKind) and kind.loss == _C.LISTWISE_LAMBDARANK:
        raise TypeError("mlp_loss_step has no LambdaRank slot: take mlp_lambdarank_step (the module: "
                        "FusedMLPLambdaRankLoss), or the Linear scorer: FusedLinearLoss, linear_loss_step, LinearScorer")
    return _mlp_step(xs, params, relevance, n, kind, sigma, grad_out, return_scores, return_loss_sum, out)


def mlp_lambdarank_step(xs, params, relevance, n, sigma=1.0, k=None, grad_out=None, return_scores=False,
                        return_loss_sum=False, out=None):
    """:func:`mlp_loss_step` for LambdaRank (:class:`pytorchltr_amd.loss.LambdaRankLoss` ``(sigma, k)``): one fused
    forward+backward step of ``LambdaRankLoss(sigma, k)(mlp(xs), relevance, n)`` without autograd, by
    ``ltr_mlp_lambdarank_f32`` (include/ltr_mlp_lambdarank.h) -- the NDCG@k swap weights and the top-k pair pass in the
    loss slot of the two fused MLP kernels.  ``k=None``: no cutoff.  The other arguments, the returned tuple and the
    shapes are those of :func:`mlp_loss_step`; off the plan (:func:`mlp_lambdarank_supported`: longer lists, a
    ``torch.bfloat16`` batch) the step runs as the three pieces -- the row score kernel, the stand-alone LambdaRank
    kernel (past ``max_list_len()`` documents its long path), the row gradient kernel."""
    from .loss import pairwise_lambda as _pl
    k = _pl.LambdaRankLoss(sigma, k).k                      # (its check of k)
    return _mlp_step(xs, params, relevance, n, _ListwiseKind(_C.LISTWISE_LAMBDARANK, k), float(sigma), grad_out,
                     return_scores, return_loss_sum, out)


def _mlp_listwise_plan(kind, B, L, F, H1, H2):
    """The `plan` of `_mlp_route` for a listwise `kind`: the plan of the entry point that has its slot."""
    if kind.loss == _C.LISTWISE_LAMBDARANK:
        return mlp_lambdarank_supported(B, L, F, H1, H2)
    return mlp_listwise_supported(kind, B, L, F, H1, H2)


_NO_TIE = (None, 0, 0, None)


def _mlp_family_call(kind, sigma, L, dev):
    """What a fused step call takes from its resolved `kind`, once for `_mlp_step` and `MLPTrainer.step`:
    ``(family, code, k, tie, entry, lead, empty_is_noop)`` -- the trainer's family and code, k clamped to the C int, the
    four tie arguments (one seed draw per call, for ListMLE only), the family's own entry point, its leading arguments,
    and whether that entry point launches nothing for an empty batch (so the caller zeroes the gradient)."""
    if not isinstance(kind, _ListwiseKind):
        return _C.MLP_TRAIN_PAIRWISE, kind, 0, _NO_TIE, "ltr_mlp_pairwise_f32", (kind, float(sigma)), False
    if kind.loss == _C.LISTWISE_LAMBDARANK:
        k = min(int(kind.k or 0), 0x7FFFFFFF)
        return _C.MLP_TRAIN_LAMBDARANK, 0, k, _NO_TIE, "ltr_mlp_lambdarank_f32", (k, float(sigma)), True
    from . import _ties
    k = int(kind.k or 0)
    tie = _ties.tie_args(_ties.draw_seed(L, dev) if kind.loss == _C.LISTWISE_LISTMLE else None)
    return _C.MLP_TRAIN_LISTWISE, kind.loss, k, tie, "ltr_mlp_listwise_f32", (kind.loss, k), True


def _mlp_step(xs, params, relevance, n, kind, sigma, grad_out, return_scores, return_loss_sum, out):
    """The step behind mlp_loss_step, mlp_lambdarank_step and the loss modules (`_MLPLossFunction`), on a resolved
    (kind, sigma): a pairwise kind, or a :class:`_ListwiseKind` of ListNet, ListMLE or LambdaRank."""
    listwise = isinstance(kind, _ListwiseKind)
    F, H1, H2 = params[0].shape[-1], params[0].shape[0], params[2].shape[0]    # (the network's: W1 is (H1, F))
    plan = not listwise or (xs.dim() == 3 and _mlp_listwise_plan(kind, xs.shape[0], xs.shape[1], F, H1, H2))
    route = _mlp_route_of("step", xs, F, H1, H2, kind, plan)
    if route is _TORCH:
        _mlp_not_taken(xs, params, True)
    X, flat_params, H1, H2, _, _ = _mlp_prepare(xs, params, _ROUTE_FAMILY[route], pad=False)
    if route is not _FUSED:
        # past the fused kernels' list lengths or listwise plan, or a bf16 batch (they are fp32-only): three pieces
        return _mlp_step_pieces(X, flat_params, H1, H2, relevance, n, kind, sigma, grad_out, return_scores,
                                return_loss_sum, out)
    B, L, F = X.shape
    dev = X.device
    r, nn = _labels_and_n(relevance, n, B, L, dev)
    lib = _C.lib()
    P, ws_bytes = _mlp_sizes_for(B, F, H1, H2)
    lossv = torch.empty(B, dtype=torch.float32, device=dev)
    flat = _mlp_grad_buffer(out, P, dev)
    # (loss_sum is written, not accumulated, by the reduction launch; B == 0 launches nothing)
    lsum = None
    if return_loss_sum:
        lsum = (torch.empty if B > 0 else torch.zeros)(1, dtype=torch.float32, device=dev)
    scores = torch.zeros(B, L, dtype=torch.float32, device=dev) if return_scores else None
    go = None if grad_out is None else grad_out.reshape(B).float().contiguous()
    family, _, _, tie, entry, lead, empty_is_noop = _mlp_family_call(kind, sigma, L, dev)
    with _C.device_ctx(X):
        st = _C.stream_of(X)
        ws = _mlp_workspace(dev, st, ws_bytes)
        if B == 0 and empty_is_noop:
            flat.zero_()                    # (the listwise and LambdaRank entry points launch nothing for an empty batch)
        rc = getattr(lib, entry)(
            *lead, X.data_ptr(), *[t.data_ptr() for t in flat_params], r.data_ptr(), _LABEL_CODE[r.dtype],
            nn.data_ptr(), *(tie if family == _C.MLP_TRAIN_LISTWISE else ()), None if go is None else go.data_ptr(),
            B, L, F, H1, H2, lossv.data_ptr(), None if scores is None else scores.data_ptr(), flat.data_ptr(),
            None if lsum is None else lsum.data_ptr(), ws.data_ptr(), ws_bytes, st)
        if rc != 0:
            _C.check(rc)
    res = (lossv, _split_grads(flat, F, H1, H2))
    if return_scores:
        res = res + (scores,)
    if return_loss_sum:
        res = res + (lsum,)
    return res


def mlp_scores(xs, params, n=None):
    """``model(xs)`` of the guide's network as one fused kernel (no autograd): (B, L) float32
    scores for documents < n[b] and 0 for the padded ones; n=None scores every document.
    Lists up to :func:`mlp_max_list_len` run the per-query kernel (ltr_mlp_scores_f32), longer ones the row kernel
    (ltr_mlp_rows_scores_f32: any length).  Feature counts and hidden sizes outside the kernels' limits raise
    ValueError (see :func:`mlp_supported`)."""
    route = _mlp_route_of("scores", xs, params[0].shape[-1], params[0].shape[0], params[2].shape[0])
    if route is _TORCH:
        _mlp_not_taken(xs, params, False)
    X, flat_params, H1, H2, _, _ = _mlp_prepare(xs, params, _MLP_ROWS, pad=False)
    fn = _mlp_query_scores if route is _PER_QUERY else _mlp_rows_scores
    return fn(X, flat_params, H1, H2, None if n is None else prepare_n(n, X.shape[0]))


def _mlp_query_scores(X, flat_params, H1, H2, nn):
    """ltr_mlp_scores_f32, the per-query score kernel, on prepared arguments: (B, L) scores, 0 on the padded documents."""
    B, L, F = X.shape
    if nn is None:
        nn = torch.full((B,), L, dtype=torch.int64, device=X.device)
    scores = torch.empty(B, L, dtype=torch.float32, device=X.device)
    if B > 0:
        with _C.device_ctx(X):
            _C.check(_C.lib().ltr_mlp_scores_f32(
                _C.ptr(X), *[_C.ptr(t) for t in flat_params], _C.ptr(nn), B, L, F, H1, H2,
                _C.ptr(scores), _C.stream_of(X)))
    return scores


def _mlp_not_taken(xs, params, got):
    """What mlp_loss_step / mlp_scores raise where `_mlp_route` finds no kernel: the prepare step's errors come first."""
    X = _prepare_features(xs)
    _, H1, H2 = _flat_params(params, X.shape[2])
    raise ValueError("fused MLP kernel takes L <= %d (F <= 144: %d), F <= %d with F %% 4 == 0, hidden <= %s"
                     % (MLP_MAX_LIST_LEN, MLP_MAX_LIST_LEN_NARROW, MLP_MAX_FEATURES, MLP_MAX_HIDDEN)
                     + ("; got L=%d F=%d hidden=(%d, %d)" % (X.shape[1], X.shape[2], H1, H2) if got else ""))


class _MLPLossFunction(torch.autograd.Function):
    """Reduced (mean / sum) loss of the fused MLP step; the kernel already produced the parameter
    gradients of the reduced loss, backward only scales them by the incoming scalar."""

    @staticmethod
    def forward(ctx, xs, relevance, n, kind_sigma, mean, *params):
        B = xs.shape[0]
        go = None if mean else torch.ones(B, dtype=torch.float32, device=xs.device)
        kind, sigma = kind_sigma
        xs, w1, extra = _zero_pad(xs, params[0], 4)
        lossv, grads, lsum = _mlp_step(xs, (w1,) + tuple(params[1:]), relevance, n, kind, sigma, go, False, True, None)
        ctx.save_for_backward(grads[0]._base)       # the flat buffer: one scale in backward
        ctx.dims = (xs.shape[2], params[0].shape[0], params[2].shape[0])
        ctx.extra = extra
        ctx.shapes = [p.shape for p in params]
        ctx.per_query = lossv
        total = lsum.reshape(())
        out = total / B if (mean and B > 0) else total
        ctx.mark_non_differentiable(lossv)
        return out, lossv

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_total, grad_unused):
        (flat,) = ctx.saved_tensors
        scaled = _crop_grads(_split_grads(flat * grad_total, *ctx.dims), ctx.extra, ctx.shapes)
        return (None, None, None, None, None) + scaled


class _KindProxy:
    """A resolved (kind, sigma) in the shape `_resolve_loss` takes a loss module in (what `loss=` accepts)."""

    def __init__(self, kind, sigma):
        self._kind = kind
        self.sigma = sigma


class _MLPLayers(torch.nn.Module):
    """What the MLP modules share: the three ``nn.Linear`` layers (``l1`` / ``l2`` / ``l3``, the state_dict of the
    guide's ``Model``) and ``mlp(xs)`` by the route `_mlp_route` names."""

    def __init__(self, in_features, hidden=(50, 10)):
        super().__init__()
        self.in_features = in_features
        self.l1 = torch.nn.Linear(in_features, hidden[0])
        self.l2 = torch.nn.Linear(hidden[0], hidden[1])
        self.l3 = torch.nn.Linear(hidden[1], 1)

    def _params(self):
        return (self.l1.weight, self.l1.bias, self.l2.weight, self.l2.bias, self.l3.weight, self.l3.bias)

    def _hidden(self):
        layers = self._modules      # (not self.l1: nn.Module.__getattr__ costs 2 us a look, and forward() is a timed path)
        return layers["l1"].out_features, layers["l2"].out_features

    def _score(self, xs, n, route):
        if route is _TORCH:
            return self.l3(torch.nn.functional.relu(self.l2(torch.nn.functional.relu(self.l1(xs)))))
        if torch.is_grad_enabled():
            return _MLPScoreFunction.apply(xs, n, *self._params())     # (backward: the family's gradient kernel)
        # evaluation: one launch (the per-query kernel up to mlp_max_list_len documents)
        X, flat_params, H1, H2, _, _ = _mlp_prepare(xs, self._params(), _ROUTE_FAMILY[route])
        fn = _mlp_query_scores if route is _PER_QUERY else _mlp_rows_scores
        return fn(X, flat_params, H1, H2, None if n is None else prepare_n(n, X.shape[0])).unsqueeze(-1)


class _FusedMLPBase(_MLPLayers):
    """What FusedMLPLoss and FusedMLPListwiseLoss share: ``score()``, the fused step where the route is `_FUSED` and the
    unfused composition (``_pieces``) where it is not."""

    def __init__(self, in_features, loss, hidden, reduction):
        if reduction not in ("mean", "sum"):
            raise ValueError("reduction must be 'mean' or 'sum'")
        super().__init__(in_features, hidden)
        self.reduction = reduction
        self.kind, self.sigma = self._resolve(loss)
        self.last_losses = None

    def score(self, xs, n=None):
        """``model(xs)``: (B, L, 1) scores (padded documents, when ``n`` is given, score 0) from the HIP kernels:
        under ``torch.no_grad()`` (evaluation) one launch -- the per-query kernel up to :func:`mlp_max_list_len`
        documents, the row kernel past it --, with gradients enabled the row score kernel, whose backward is the row
        gradient kernel (:class:`MLPScorer`).  Rows wider than 224 features, up to 704, take the wide-row kernels
        (ltr_mlp_wide_*_f32) in both cases, at every list length.  The three ``nn.Linear`` layers, with autograd, serve
        what those do not take: more than 704 features, hidden sizes past (64, 16), features that require a gradient,
        other dtypes, autocast.  A ``torch.bfloat16`` batch (outside autocast, no gradient of its own) runs the bf16
        kernels (ltr_mlp_bf16_*: W1 rounded to bf16 for the first layer, fp32 behind it) at every list length, with
        and without gradients; more than 224 features (after padding to 8) or hidden sizes past (64, 16) raise
        ValueError there."""
        return self._score(xs, n, _mlp_route_of("score", xs, None, *self._hidden()))

    def _plan(self, B, L, F4, H1, H2):
        """The `plan` of `_mlp_route`: the pairwise fused step has none beyond :func:`mlp_supported`."""
        return True

    def _fused_shape(self, B, L, F4):
        return mlp_supported(L, F4, *self._hidden()) and self._plan(B, L, F4, *self._hidden())

    def forward(self, xs, relevance, n):
        _C.require_device(xs, "xs")
        B, L, F = xs.shape
        H1, H2 = self._hidden()
        route = _mlp_route_of("loss", xs, F, H1, H2, self.kind, self._plan(B, L, _f4(F), H1, H2))
        if route is _FUSED:
            total, per_query = _MLPLossFunction.apply(
                xs, relevance, n, (self.kind, self.sigma), self.reduction == "mean", *self._params())
            self.last_losses = per_query
            return total
        per_query = self._pieces(self._score(xs, n, route), relevance, n)
        self.last_losses = per_query.detach()
        return per_query.mean() if self.reduction == "mean" else per_query.sum()


class FusedMLPLoss(_FusedMLPBase):
    """The guide's scorer and loss as one module: ``l1``/``l2``/``l3`` are ordinary
    ``torch.nn.Linear`` layers (state_dict-compatible with the ``Model`` class of
    docs/source/getting-started.rst:40-50), and ``forward(xs, relevance, n)`` returns the
    *reduced* loss ``loss_fn(model(xs), relevance, n).mean()`` (or ``.sum()``) whose backward
    fills the six parameter gradients -- computed by one fused MFMA kernel.

    Feature counts that are not a multiple of 4 are zero-padded on the fly.  Shapes the kernel
    does not take run as the unfused composition.  Lists longer than 256 (128 beyond 144 features), of any length:
    the row score kernel, the HIP loss kernel and the row gradient kernel (ltr_mlp_rows_*_f32, :class:`MLPScorer`) --
    a loss module built with ``long_lists=True`` takes them past ``max_list_len()`` documents.  More than 224
    features, up to 704 (Yahoo: 699), at every list length: the same three pieces on the wide-row kernels
    (ltr_mlp_wide_*_f32).  A ``torch.bfloat16`` batch (up to 224 features): the same three pieces on the bf16 kernels
    (ltr_mlp_bf16_*, :func:`mlp_scores_bf16`) at every list length -- the one-launch fused step is fp32-only.  More than 704 features or hidden sizes past (64, 16): the torch layers + the HIP loss kernel.  ``score(xs)`` evaluates the
    network alone (for the metrics).  The seven pairwise losses; the listwise ones: :class:`FusedMLPListwiseLoss`.
    """

    def __init__(self, in_features, loss="hinge", hidden=(50, 10), reduction="mean"):
        super().__init__(in_features, loss, hidden, reduction)

    _resolve = staticmethod(_resolve_pairwise_loss)

    def _pieces(self, scores, relevance, n):
        return _pairwise_pieces(scores, relevance, n, self.kind, self.sigma)


def _resolve_listwise_loss(loss):
    kind, sigma = _resolve_loss(loss)
    if not isinstance(kind, _ListwiseKind) or kind.loss == _C.LISTWISE_LAMBDARANK:       # (LambdaRank has a class of its own)
        raise TypeError("FusedMLPListwiseLoss takes the listwise losses only (\"listnet\" / \"softmax\", \"listmle\", "
                        "ListwiseSoftmaxLoss, ListMLELoss); the pairwise ones: FusedMLPLoss; LambdaRank: "
                        "FusedMLPLambdaRankLoss")
    return kind, sigma


class FusedMLPListwiseLoss(_FusedMLPBase):
    """:class:`FusedMLPLoss` for the listwise losses: ``loss`` is ``"listnet"`` (``"softmax"``), ``"listmle"``,
    ``ListwiseSoftmaxLoss()`` or ``ListMLELoss(k)``.  Same layers, ``state_dict``, ``score()``, ``last_losses`` and
    feature padding; the fused step is ``ltr_mlp_listwise_f32`` (include/ltr_listwise.h), ListNet or ListMLE in the
    loss slot of the same two MFMA kernels.  Shapes its plan declines run as the unfused composition of ``score()``
    with autograd and the stand-alone listwise loss kernel: lists longer than 256 (128 beyond 144 features), ListMLE
    at any length, on the row score and row gradient kernels (ltr_mlp_rows_*_f32); more than 224 features, up to 704,
    at every list length on the wide-row kernels (ltr_mlp_wide_*_f32); hidden sizes past (64, 16) or more than 704
    features on the torch layers.  ListMLE breaks label ties as :class:`pytorchltr_amd.loss.ListMLELoss` does."""

    def __init__(self, in_features, loss="listnet", hidden=(50, 10), reduction="mean"):
        super().__init__(in_features, loss, hidden, reduction)

    _resolve = staticmethod(_resolve_listwise_loss)

    def _plan(self, B, L, F4, H1, H2):
        return mlp_listwise_supported(self.kind, B, L, F4, H1, H2)

    def _pieces(self, scores, relevance, n):
        return _listwise_pieces(scores, relevance, n, self.kind)


class FusedMLPLambdaRankLoss(_FusedMLPBase):
    """:class:`FusedMLPLoss` for LambdaRank, the NDCG@k objective of :class:`pytorchltr_amd.loss.LambdaRankLoss`:
    ``sigma`` and ``k`` (``None``: no cutoff) are that loss's, or come from a ``LambdaRankLoss`` module passed as
    ``loss``.  Same layers, ``state_dict``, ``score()``, ``last_losses`` and feature padding; the fused step is
    ``ltr_mlp_lambdarank_f32`` (include/ltr_mlp_lambdarank.h), the row function of the stand-alone LambdaRank kernel in
    the loss slot of the same two MFMA kernels.  Shapes its plan declines (:func:`mlp_lambdarank_supported`) run as the
    unfused composition of ``score()`` with autograd and the stand-alone kernel, as for :class:`FusedMLPListwiseLoss`;
    lists past ``max_list_len()`` documents, up to ``max_pair_list_len()``, take that kernel's long path."""

    def __init__(self, in_features, loss=None, sigma=1.0, k=None, hidden=(50, 10), reduction="mean"):
        from .loss import pairwise_lambda as _pl
        if loss is None:
            loss = _pl.LambdaRankLoss(sigma, k)             # (its check of k)
        elif not isinstance(loss, _pl.LambdaRankLoss):
            raise TypeError("FusedMLPLambdaRankLoss takes a LambdaRankLoss module, or sigma and k (the pairwise losses: "
                            "FusedMLPLoss; ListNet and ListMLE: FusedMLPListwiseLoss)")
        super().__init__(in_features, loss, hidden, reduction)

    _resolve = staticmethod(_resolve_loss)

    def _plan(self, B, L, F4, H1, H2):
        return mlp_lambdarank_supported(B, L, F4, H1, H2)

    def _pieces(self, scores, relevance, n):
        return _listwise_pieces(scores, relevance, n, self.kind, self.sigma)


class MLPScorer(_MLPLayers):
    """The guide's scorer ``Linear(F, H1) / ReLU / Linear(H1, H2) / ReLU / Linear(H2, 1)`` on its own -- what
    :class:`LinearScorer` is to ``nn.Linear(F, 1)``: ``loss_fn(scorer(xs), ys, n)`` with any loss, at any list length.
    ``l1`` / ``l2`` / ``l3`` are ordinary ``torch.nn.Linear`` layers (the state_dict of :class:`FusedMLPLoss` and of
    the guide's ``Model``).  ``forward(xs, n=None)`` returns (B, L, 1) scores from the row score kernel
    (ltr_mlp_rows_scores_f32; with ``n`` the padded documents score 0 and their features are not read); its backward
    runs the row gradient kernel on ``grad_scores`` and fills the six ``.grad``s (activations are recomputed, nothing
    but the features is kept).  Feature counts that are not a multiple of 4 are zero-padded on the fly.  Features
    that require a gradient, inputs that are neither fp32 nor bf16, more than 704 features or hidden sizes past (64, 16)
    run the torch layers; a ``torch.bfloat16`` batch runs the bf16 kernels (ltr_mlp_bf16_*, :func:`mlp_scores_bf16`:
    half the bytes, W1 rounded to bf16 for the first layer; up to 224 features, ValueError past that); 228 to 704 features (Yahoo: 699, padded to 700) run the wide-row kernels (ltr_mlp_wide_*_f32), which
    stream the feature dimension in chunks.  CPU tensors are refused: there is no CPU fallback."""

    def forward(self, xs, n=None):
        _C.require_device(xs, "xs")
        return self._score(xs, n, _mlp_route_of("scorer", xs, None, *self._hidden()))


# ---- MLPTrainer: the fused MLP step with the optimizer update inside the reduction launch (include/ltr_mlp_train.h) ----
_TRAIN_ALGO = {"sgd": _C.OPT_SGD, "adagrad": _C.OPT_ADAGRAD, "adam": _C.OPT_ADAM}
_TRAIN_TORCH = {"sgd": "SGD", "adagrad": "Adagrad", "adam": "Adam"}
_TRAIN_STATE_NAMES = {"sgd": ("momentum_buffer",), "adagrad": ("sum",), "adam": ("exp_avg", "exp_avg_sq")}
_TRAIN_REFUSED = ("maximize", "amsgrad", "differentiable")
_TRAIN_IGNORED = ("foreach", "capturable", "fused")             # how torch runs its own kernels: nothing to choose here


def _train_hyper(optimizer, lr, hyper):
    """The hyper-parameters of `optimizer` as torch.optim holds them (its names, defaults and ValueErrors: the torch
    class itself judges them, on a parameter of its own that is never stepped)."""
    if optimizer not in _TRAIN_ALGO:
        raise ValueError("optimizer must be 'sgd', 'adagrad' or 'adam'; got %r" % (optimizer,))
    hyper = dict(hyper)
    for name in _TRAIN_REFUSED:
        if hyper.pop(name, False):
            raise NotImplementedError("MLPTrainer has no %s=True (torch.optim.%s on model.parameters() has)"
                                      % (name, _TRAIN_TORCH[optimizer]))
    for name in _TRAIN_IGNORED:
        hyper.pop(name, None)
    if lr is not None:
        hyper["lr"] = lr
    if torch.is_tensor(hyper.get("lr")):
        raise ValueError("MLPTrainer takes lr as a number (a tensor lr belongs to torch's capturable optimizers)")
    probe = getattr(torch.optim, _TRAIN_TORCH[optimizer])([torch.zeros(1, requires_grad=True)], **hyper)
    return {k: v for k, v in probe.defaults.items() if k not in _TRAIN_REFUSED + _TRAIN_IGNORED}


def _train_param_shapes(F, H1, H2):
    return ((H1, F), (H1,), (H2, H1), (H2,), (1, H2), (1,))


def mlp_train_state_to_torch(optimizer, flat, t, F, H1, H2, w1_cols=None, initial=False):
    """The ``state`` of the matching torch.optim optimizer's state_dict (parameter index -> its state) from the
    trainer's flat state: `flat` holds the buffers of include/ltr_mlp_train.h back to back (one of P floats, Adam two,
    each laid out [W1 | b1 | W2 | b2 | W3 | b3] with W1 rows of F floats, of which the first `w1_cols` are the
    parameter's), `t` the step count.  A pure function on tensors (any device).  Where torch has no state yet -- SGD
    without momentum or before its first step, Adam before its first step -- the dict is empty."""
    names = _TRAIN_STATE_NAMES[optimizer]
    P = sum(a * b for a, b in ((H1, F), (H1, 1), (H2, H1), (H2, 1), (H2, 1), (1, 1)))
    if optimizer != "adagrad" and (t == 0 or flat is None):
        return {}
    out = {i: {} for i in range(6)}
    for b, name in enumerate(names):
        parts = _crop_grads(_split_grads(flat[b * P:(b + 1) * P], F, H1, H2), F - (w1_cols or F))
        for i, (part, shape) in enumerate(zip(parts, _train_param_shapes(w1_cols or F, H1, H2))):
            out[i][name] = part.reshape(shape).clone()
    if optimizer != "sgd":
        for i in range(6):
            out[i]["step"] = torch.tensor(float(t))
    return out


def mlp_train_state_from_torch(optimizer, state, F, H1, H2, w1_cols=None, fill=0.0, device=None):
    """The inverse of :func:`mlp_train_state_to_torch`: ``(flat, t)`` from the ``state`` of a torch.optim state_dict
    (keys 0 .. 5 in the order of ``model.parameters()``; an empty or partial state counts as "no step taken": the
    buffers hold `fill`).  W1's state is zero-padded from `w1_cols` columns to rows of F floats."""
    names = _TRAIN_STATE_NAMES[optimizer]
    shapes = _train_param_shapes(w1_cols or F, H1, H2)
    P = sum(a * b for a, b in ((H1, F), (H1, 1), (H2, H1), (H2, 1), (H2, 1), (1, 1)))
    have = all(i in state and all(state[i].get(name) is not None for name in names) for i in range(6))
    flat = torch.full((len(names) * P,), float(fill), dtype=torch.float32, device=device)
    if not have:
        return flat, 0
    for b, name in enumerate(names):
        pieces = []
        for i, shape in enumerate(shapes):
            v = state[i][name].detach().to(device=device, dtype=torch.float32)
            if tuple(v.shape) != shape:
                raise ValueError("state %r of parameter %d has shape %s, not %s" % (name, i, tuple(v.shape), shape))
            if i == 0 and shape[1] != F:
                v = torch.nn.functional.pad(v, (0, F - shape[1]))
            pieces.append(v.reshape(-1))
        flat[b * P:(b + 1) * P] = torch.cat(pieces)
    if optimizer == "sgd":
        return flat, 1                       # (torch keeps no count: a momentum buffer means "not the first step")
    steps = {int(float(state[i]["step"])) for i in range(6)}
    if len(steps) != 1:
        raise ValueError("the six parameters' step counts differ: %s" % sorted(steps))
    return flat, steps.pop()


class MLPTrainer:
    """The guide's loop body -- ``zero_grad / loss / backward / optimizer.step`` -- on a fused MLP loss module as ONE
    call without autograd: ``loss = trainer.step(xs, relevance, n)`` runs the module's fused step with the optimizer
    update and its state inside the reduction launch (ltr_mlp_train_step_f32: two launches), and returns the reduced
    loss as a 0-dim device tensor.

    Args:
        model: a :class:`FusedMLPLoss`, :class:`FusedMLPListwiseLoss` or :class:`FusedMLPLambdaRankLoss` on the device;
            its loss, sigma, k and reduction are read at every step, its six ``nn.Linear`` parameters (fp32) are
            updated in place -- no autograd graph, no ``.grad``.
        optimizer: ``"sgd"``, ``"adagrad"`` or ``"adam"``; `lr` and the keyword hyper-parameters are those of
            ``torch.optim.SGD / Adagrad / Adam`` (names, defaults, ValueErrors).  ``maximize``, ``amsgrad`` and
            ``differentiable`` raise NotImplementedError; ``foreach``, ``capturable`` and ``fused`` mean nothing here.

    ``trainer.lr`` is a plain attribute, read at every eager step (schedulers set it).  ``state_dict()`` /
    ``load_state_dict()`` speak the format of the matching torch optimizer built on ``model.parameters()``, in both
    directions.  Batches off the fused route (longer lists, wide rows, bf16, a listwise loss off its plan) run the
    pieces of :func:`mlp_loss_step` into a flat gradient and one update launch (ltr_mlp_apply_update_f32); shapes no
    kernel takes raise the ValueError of :func:`mlp_loss_step`.  The tensors `step` returns (the loss, ``last_losses``,
    the gradient views) are buffers of the trainer, overwritten by the next step on the same shape."""

    def __init__(self, model, optimizer="adagrad", lr=None, **hyper):
        if not isinstance(model, _FusedMLPBase):
            raise TypeError("MLPTrainer takes a FusedMLPLoss, FusedMLPListwiseLoss or FusedMLPLambdaRankLoss module")
        self.model = model
        self.optimizer = optimizer
        self.hyper = _train_hyper(optimizer, lr, hyper)
        self.lr = self.hyper.pop("lr")
        self._optim = _C.MLPOptim()
        self._state = None               # the flat state of include/ltr_mlp_train.h (device), made at the first step
        self._pending = None             # a loaded state (torch's form) waiting for the device
        self._buffers = {}               # (B, L, F) -> the step's loss / total / weight / workspace / gradient buffers

    # -- the network and its state --
    def _dims(self):
        H1, H2 = self.model._hidden()
        return self.model.in_features, H1, H2

    def _params(self):
        params = self.model._params()
        for p in params:
            if p.dtype is not torch.float32 or not p.is_contiguous() or not p.is_cuda:
                raise ValueError("MLPTrainer updates contiguous float32 parameters on the device in place")
        return params

    def _fill(self):
        return float(self.hyper.get("initial_accumulator_value", 0.0))

    def _state_for(self, Fp, dev):
        """The flat state for rows of Fp floats on `dev`: zeroed (Adagrad: `sum` at its initial value), or what was
        loaded; a state made for another row width or device is carried over through torch's form."""
        if self._state is not None and self._state_Fp == Fp and self._state.device == dev:
            return self._state
        F, H1, H2 = self._dims()
        source = self._torch_state() if self._state is not None else (self._pending or {})
        flat, t = mlp_train_state_from_torch(self.optimizer, source, Fp, H1, H2, F, self._fill(), dev)
        count = int(_C.lib().ltr_mlp_train_state_floats(_TRAIN_ALGO[self.optimizer], Fp, H1, H2))
        state = torch.zeros(count, dtype=torch.float32, device=dev)
        state[:flat.numel()] = flat
        state[count - 4:].view(torch.int32)[0] = int(t)
        self._state, self._state_Fp, self._pending = state, Fp, None
        return state

    @property
    def steps(self):
        """The number of steps taken: the device counter (a host read: it synchronises).  Adagrad and Adam carry it
        through a loaded state_dict and through a change of the batch's row width (fp32 and bf16 batches pad the
        features differently, and the flat state is re-laid through torch's form).  torch's SGD state holds no count,
        so after either the SGD count restarts: 1 where a momentum buffer came along, else 0 -- all the first-step
        rule asks is whether t is 0, which it cannot tell from the truth."""
        if self._state is None:
            return 0 if self._pending is None else mlp_train_state_from_torch(
                self.optimizer, self._pending, *self._dims())[1]
        return int(self._state[-4:].view(torch.int32)[0].item())

    def _torch_state(self):
        if self._state is None:
            if self._pending is not None:
                return self._pending
            F, H1, H2 = self._dims()
            if self.optimizer != "adagrad":
                return {}
            P = int(sum(a * b for a, b in ((H1, F), (H1, 1), (H2, H1), (H2, 1), (H2, 1), (1, 1))))
            return mlp_train_state_to_torch("adagrad", torch.full((P,), self._fill()), 0, F, H1, H2)
        F, H1, H2 = self._dims()
        state = mlp_train_state_to_torch(self.optimizer, self._state, self.steps, self._state_Fp, H1, H2, F)
        if self.optimizer == "sgd" and self.hyper["momentum"] == 0:
            return {}
        return state

    def _param_groups(self):
        probe = getattr(torch.optim, _TRAIN_TORCH[self.optimizer])(
            [torch.zeros(1, requires_grad=True) for _ in range(6)], lr=self.lr, **self.hyper)
        return probe.state_dict()["param_groups"]

    def state_dict(self):
        """The state_dict of ``torch.optim.<Optimizer>(model.parameters(), ...)`` at this point: same keys, parameter
        order and per-parameter names (``momentum_buffer``; ``sum``, ``step``; ``exp_avg``, ``exp_avg_sq``, ``step``).
        Reads the device step counter (synchronises)."""
        return {"state": self._torch_state(), "param_groups": self._param_groups()}

    def load_state_dict(self, state_dict):
        """Takes a state_dict of this class or of the matching torch.optim optimizer on ``model.parameters()``: the
        per-parameter state and the group's hyper-parameters (``lr`` included).  The state holds no entry (no step
        taken) or the six parameters'; any other count is a ValueError, and the trainer stays as it was."""
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != 6:
            raise ValueError("MLPTrainer takes one parameter group of the model's six parameters")
        group = {k: v for k, v in groups[0].items() if k != "params"}
        for name in _TRAIN_REFUSED:
            if group.get(name):
                raise NotImplementedError("MLPTrainer has no %s=True" % name)
        keys = sorted(state_dict["state"])
        if len(keys) not in (0, 6):                # (refused before anything of the trainer changes)
            raise ValueError("the state holds %d per-parameter entries; MLPTrainer takes none (no step taken) or the "
                             "model's six" % len(keys))
        hyper = _train_hyper(self.optimizer, None, {k: v for k, v in group.items() if k in dict(self.hyper, lr=0)})
        self.lr = hyper.pop("lr")
        self.hyper = hyper
        # (copies: the dict's own tensors stay the caller's -- a torch optimizer that loaded it steps them in place)
        state = {i: {name: v.detach().clone() if torch.is_tensor(v) else v for name, v in state_dict["state"][k].items()}
                 for i, k in enumerate(keys)} if len(keys) == 6 else {}
        F, H1, H2 = self._dims()
        mlp_train_state_from_torch(self.optimizer, state, F, H1, H2)        # (its shape checks, now)
        self._state, self._pending = None, state

    # -- the step --
    def _fill_optim(self):
        o, h = self._optim, self.hyper
        o.algo = _TRAIN_ALGO[self.optimizer]
        o.lr = float(self.lr)
        o.weight_decay = float(h["weight_decay"])
        o.nesterov = 1 if h.get("nesterov") else 0
        o.momentum, o.dampening = float(h.get("momentum", 0.0)), float(h.get("dampening", 0.0))
        o.lr_decay, o.eps = float(h.get("lr_decay", 0.0)), float(h.get("eps", 0.0))
        o.beta1, o.beta2 = [float(b) for b in h.get("betas", (0.0, 0.0))]
        return o

    def _buffers_for(self, B, L, Fp, H1, H2, dev):
        key = (B, L, Fp, dev.index)
        buf = self._buffers.get(key)
        if buf is None:
            P, ws_bytes = _mlp_sizes_for(B, Fp, H1, H2)
            if len(self._buffers) > 16:
                self._buffers.clear()
            buf = self._buffers[key] = dict(
                loss=torch.empty(B, dtype=torch.float32, device=dev), lsum=torch.empty(1, dtype=torch.float32, device=dev),
                total=torch.empty((), dtype=torch.float32, device=dev), ones=torch.ones(B, dtype=torch.float32, device=dev),
                ws=torch.empty(max(ws_bytes, 16) // 4, dtype=torch.float32, device=dev), ws_bytes=ws_bytes,
                grads=torch.empty(P, dtype=torch.float32, device=dev), P=P)
        return buf

    def _prime(self, xs):
        """The state and the buffers of a batch shape, made ahead of a capture (their initialisation must not be
        replayed: it would reset the step count)."""
        B, L, F = xs.shape
        H1, H2 = self.model._hidden()
        Fp = F + (-F) % (8 if xs.dtype is torch.bfloat16 else 4)
        self._state_for(Fp, xs.device)
        if B > 0:
            self._buffers_for(B, L, Fp, H1, H2, xs.device)

    def step(self, xs, relevance, n, return_grads=False):
        """One training step on a batch: the reduced loss (a 0-dim device tensor), and with ``return_grads=True`` also
        the six gradient views ``(dW1, db1, dW2, db2, dW3, db3)`` of the gradient the update consumed.  Sets
        ``model.last_losses``.  An empty batch changes nothing and returns 0.  Never synchronises; on the fused route it
        allocates nothing after the first call on a shape, so ``torch.cuda.graph`` captures it (:meth:`graphed`)."""
        model = self.model
        _C.require_device(xs, "xs")
        if xs.dim() != 3:
            raise ValueError("features must have shape (batch, list_size, features)")
        params = self._params()
        B, L, F = xs.shape
        H1, H2 = model._hidden()
        dev = xs.device
        if params[0].shape[1] != F:
            raise ValueError("the model takes %d features, the batch has %d" % (params[0].shape[1], F))
        kind, sigma, mean = model.kind, model.sigma, model.reduction == "mean"
        if B == 0:
            model.last_losses = torch.zeros(0, dtype=torch.float32, device=dev)
            zero = torch.zeros((), dtype=torch.float32, device=dev)
            return (zero, tuple(torch.zeros_like(p) for p in params)) if return_grads else zero
        xp, w1p, extra = _zero_pad(xs, params[0], 8 if xs.dtype is torch.bfloat16 else 4)
        Fp = F + extra
        listwise = isinstance(kind, _ListwiseKind)
        plan = not listwise or _mlp_listwise_plan(kind, B, L, Fp, H1, H2)
        route = _mlp_route_of("step", xp, Fp, H1, H2, kind, plan)
        if route is _TORCH and _mlp_route_of("loss", xp, Fp, H1, H2, kind, plan) is _WIDE:
            route = _WIDE                                   # (the module's wide rows: the functions have no such route)
        step_params = (w1p,) + tuple(params[1:])
        if route is _TORCH:
            _mlp_not_taken(xp, step_params, True)
        X, flat_params, H1, H2, _, _ = _mlp_prepare(xp, step_params, _ROUTE_FAMILY[route], pad=False)
        state = self._state_for(Fp, dev)
        optim = self._fill_optim()
        buf = self._buffers_for(B, L, Fp, H1, H2, dev)
        lib = _C.lib()
        if route is not _FUSED:
            lossv, _, lsum = _mlp_step_pieces(X, flat_params, H1, H2, relevance, n, kind, sigma,
                                              None if mean else buf["ones"], False, True, buf["grads"])
            with _C.device_ctx(X):
                _C.check(lib.ltr_mlp_apply_update_f32(
                    buf["grads"].data_ptr(), *[p.data_ptr() for p in params], F, state.data_ptr(), ctypes.byref(optim),
                    Fp, H1, H2, _C.stream_of(X)))
            buf["lsum"].copy_(lsum)
        else:
            r, nn = _labels_and_n(relevance, n, B, L, dev)
            lossv = buf["loss"]
            family, code, k, tie = _mlp_family_call(kind, sigma, L, dev)[:4]
            with _C.device_ctx(X):
                rc = lib.ltr_mlp_train_step_f32(
                    family, code, k, float(sigma), X.data_ptr(), *[p.data_ptr() for p in params], F,
                    flat_params[0].data_ptr() if extra else None, r.data_ptr(), _LABEL_CODE[r.dtype], nn.data_ptr(),
                    *tie, None if mean else buf["ones"].data_ptr(), B, L, Fp, H1, H2, lossv.data_ptr(), None,
                    buf["lsum"].data_ptr(), state.data_ptr(), ctypes.byref(optim),
                    buf["grads"].data_ptr() if return_grads else None, buf["ws"].data_ptr(), buf["ws_bytes"],
                    _C.stream_of(X))
                if rc != 0:
                    _C.check(rc)
        model.last_losses = lossv
        if mean:
            total = torch.div(buf["lsum"].view(()), B, out=buf["total"])
        else:
            total = buf["lsum"].view(())
        if return_grads:
            return total, _crop_grads(_split_grads(buf["grads"], Fp, H1, H2), extra, [p.shape for p in params])
        return total

    def graphed(self, example_batch, warmup=3):
        """``trainer.step`` on batches of one shape as a captured graph: returns a callable like
        :class:`pytorchltr_amd.graphed.GraphedStep`'s -- ``loss = call(xs, relevance, n)`` copies the batch into static
        buffers, replays the two launches and returns the static 0-dim loss.  `warmup` eager steps on `example_batch`
        run first and DO update the parameters.  The step counter lives on the device, so Adam's and Adagrad's
        t-dependent factors and SGD's first-step rule replay correctly; the learning rate is a kernel argument and
        stays at the value ``trainer.lr`` had at capture -- capture again after changing it."""
        return _GraphedTrainerStep(self, example_batch, warmup)


class _GraphedTrainerStep:
    def __init__(self, trainer, example_batch, warmup):
        self._trainer = trainer
        self._static = [t.clone() for t in example_batch]
        if len(self._static) != 3 or not self._static[0].is_cuda:
            raise ValueError("graphed() needs the device tensors (xs, relevance, n) of an example batch")
        trainer._params()
        trainer._prime(self._static[0])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(0, warmup)):
                trainer.step(*self._static)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph, capture_error_mode="thread_local"):
            self._loss = trainer.step(*self._static)
        torch.cuda.synchronize()
        self._keep = (trainer._state, list(trainer._buffers.values()))      # what the graph's launches point into

    def __call__(self, *batch):
        if len(batch) != len(self._static):
            raise ValueError("expected %d tensors, got %d" % (len(self._static), len(batch)))
        for dst, src in zip(self._static, batch):
            if dst.shape != src.shape:
                raise ValueError("batch shape %s differs from the captured shape %s (pad batches "
                                 "to a fixed list size)" % (tuple(src.shape), tuple(dst.shape)))
            dst.copy_(src, non_blocking=True)
        self._graph.replay()
        return self._loss
